"""tests/merge_cases.py on the CPU: the builder round-trips through the numpy restatements of both wire forms without ever
reading a dead word, its expectation is the oracle's merge (and a hand-computed answer), the gloo test double merges the
built buffers the same way, and the comparison the GPU tests use fails on three deliberately wrong results."""
import numpy as np
import pytest

import merge_cases as mc
from cpu_pipeline import OraclePipeline, decode_wire, unpack_wire
from renderer_amd.pipeline import DRAW_CMD_DTYPE

TABLES = list(mc.TABLE_SIZES)
ENTRIES = list(mc.CATALOGUE)


def test_the_catalogue_has_every_family_the_merge_kernels_branch_on():
    assert {mc.family(n) for n in ENTRIES} == {"single", "align", "empty", "chunks", "wrap", "packed"}
    assert [mc.CATALOGUE[f"single-{c}"]["counts"] for c in mc.SINGLE] == [[c] for c in mc.SINGLE]
    # the chunk that starts mid-quad: its destination's word offset 5 * count_base takes every residue modulo 4
    assert {5 * c0 % 4 for c0 in mc.ALIGN_C0} == {0, 1, 2, 3} and {5 * (c0 + 300) % 4 for c0 in mc.ALIGN_C0} == {0, 1, 2, 3}
    assert [len(mc.CATALOGUE[f"chunks-{n}"]["counts"]) for n in mc.N_CHUNKS] == mc.N_CHUNKS
    assert all(0 in mc.CATALOGUE[f"chunks-{n}"]["counts"] for n in (31, 32, 33, 63, 64))
    assert max(len(s["counts"]) for s in mc.CATALOGUE.values()) == 64


@pytest.mark.parametrize("table_name", TABLES)
def test_tables_and_lists_are_what_a_frame_can_emit(table_name):
    t = mc.table(table_name)
    if table_name != "scene64":
        assert (t["n_lods"] == 1).any() and (t["vertex_offset"] < 0).any()
        assert len(t) < 3 or len(np.unique(t["index_len"][:, 0])) > 1
    lists, _ = mc.case("chunks-9", table_name)
    for l in lists:
        c = l.cmds
        assert np.all(c["instanceCount"] == 1) and np.all(c["indexCount"] > 0)
        assert np.all(np.diff(c["firstInstance"].astype(np.int64)) > 0)
        assert np.all(l.far[t["n_lods"][l.mesh] == 1] == 0)
        assert np.array_equal(c["indexCount"], t["index_len"][l.mesh, l.far]) and np.array_equal(c["vertexOffset"], t["vertex_offset"][l.mesh])
        run = np.cumsum(c["indexCount"].astype(np.uint64))
        assert np.array_equal(c["firstIndex"], ((run - c["indexCount"] + np.uint64(77)) & np.uint64(mc.MASK)).astype(np.uint32))
        assert l.total == (int(run[-1]) & mc.MASK if len(c) else 0)


def test_the_wrapping_and_packed_entries_do_what_their_names_say():
    for table_name in TABLES:
        bits = mc.wire_index_bits(mc.TABLE_SIZES[table_name])
        lists, totals = mc.case("wrap-inside-a-chunk", table_name)
        fi = lists[0].cmds["firstIndex"].astype(np.int64)
        assert fi[0] == mc.WRAP_BASE and (np.diff(fi) < 0).sum() == 1, "wraps once inside the chunk"
        lists, totals = mc.case("wrap-between-chunks", table_name)
        want = mc.expected_merge(lists, totals, 257)
        assert sum(totals[:2]) < 1 << 32 < sum(totals[:3]) and want.index_total == sum(totals) & mc.MASK
        lists, totals = mc.case("wrap-in-the-index-total", table_name)
        assert sum(totals) >= 1 << 32
        lists, totals = mc.case("packed-largest-index", table_name)
        for k, l in enumerate(lists):
            rec = mc.body_of(mc.build_chunks(lists, totals, "packed", 129), k, mc.stride_for(129, "packed"))
            last = len(l.cmds) - 1
            word = int(rec[last // 64 * 68 + 4 + last % 64])
            assert word & ((1 << bits) - 1) == (1 << bits) - 1, "every bit of the index field"
        lists, totals = mc.case("packed-base-wraps", table_name)
        fi = lists[0].cmds["firstInstance"].astype(np.int64)
        assert fi[0] > 0xFFFFFFF0 - 1 and fi[-1] < fi[0], "base + index wraps u32"


# ---- builder round trip ----

@pytest.mark.parametrize("dead_fill", [0, mc.DEAD_FILL, 0xFFFFFFFF], ids=["zero", "deadbeef", "ones"])
@pytest.mark.parametrize("form", ["wire", "packed"])
@pytest.mark.parametrize("table_name", TABLES)
def test_built_bodies_decode_to_the_lists_whatever_the_dead_words_hold(table_name, form, dead_fill):
    tbl = mc.table(table_name)
    for name in ENTRIES:
        lists, totals = mc.case(name, table_name)
        cap = mc.capacity_of(lists)
        stride = mc.stride_for(cap, form)
        buf = mc.build_chunks(lists, totals, form, cap, dead_fill=dead_fill)
        assert len(buf) == len(lists) * stride // 4
        for k, l in enumerate(lists):
            head = buf[k * stride // 4:k * stride // 4 + 8]
            assert head[0] == len(l.cmds) and head[1] == totals[k] and np.all(head[2:] == dead_fill)
            body = mc.body_of(buf, k, stride)
            n = len(l.cmds)
            got = decode_wire(unpack_wire(body, n) if form == "packed" else body, n, tbl)
            assert got.tobytes() == l.cmds.tobytes(), (name, k)
        if dead_fill:   # the fill really is everywhere the header leaves unspecified: a changed fill changes only those words
            other = mc.build_chunks(lists, totals, form, cap, dead_fill=dead_fill ^ 0x55555555)
            diff = buf != other
            assert np.all(buf[diff] == dead_fill) and (diff.any() or all(len(l.cmds) == cap and cap % 256 == 0 for l in lists))


def test_the_twenty_byte_form_and_a_list_longer_than_the_stride():
    lists, totals = mc.case("align-5", "scene64")
    buf = mc.build_chunks(lists, totals, "cmds", 300)
    stride = mc.stride_for(300, "cmds")
    for k, l in enumerate(lists):
        n = len(l.cmds)
        assert mc.body_of(buf, k, stride)[:5 * n].tobytes() == l.cmds.tobytes()
        assert np.all(mc.body_of(buf, k, stride)[5 * n:] == mc.DEAD_FILL)
    for form in mc.FORMS:   # a tightened slice: the header keeps the full count, the body is what the stride holds
        cut = mc.build_chunks(lists, totals, form, 100)
        s = mc.stride_for(100, form)
        assert len(cut) == 3 * s // 4 and cut[s // 4] == 300
        full = mc.build_chunks(lists, totals, form, 300)
        whole = {"cmds": 5, "wire": 516, "packed": 68}[form]
        keep = (s // 4 - 8) // whole * whole
        assert np.array_equal(mc.body_of(cut, 1, s)[:keep], mc.body_of(full, 1, mc.stride_for(300, form))[:keep])
        assert np.all(mc.body_of(cut, 1, s)[keep:] == mc.DEAD_FILL)
    forged = mc.build_chunks(lists, totals, "wire", 300, header_counts=[None, 0xFFFFFFFF, None])
    assert forged[mc.stride_for(300, "wire") // 4] == 0xFFFFFFFF and forged[0] == 5


# ---- the expectation ----

def _cmd(index_count, first_index, vertex_offset, first_instance):
    return (index_count, 1, first_index, vertex_offset, first_instance)


def test_expected_merge_known_answer():
    """Three tiny chunks, by hand. Chunk 0 starts 6 short of 2^32 and reports 0xFFFFFFFE indices (a wrapped total of a larger
    frame), chunk 1 is empty but reports 10, chunk 2 has three commands of which a capacity of 2 keeps two."""
    a = np.array([_cmd(6, 0xFFFFFFFA, -3, 10), _cmd(9, 0x00000000, 5, 12)], DRAW_CMD_DTYPE)
    b = np.zeros(0, DRAW_CMD_DTYPE)
    c = np.array([_cmd(3, 100, 0, 40), _cmd(12, 103, 7, 41), _cmd(6, 115, 7, 45)], DRAW_CMD_DTYPE)
    totals = [0xFFFFFFFE, 10, 21]
    want = mc.expected_merge([a, b, c], totals, 3)
    # rebase of chunk 2 = 0xFFFFFFFE + 10 = 8 (mod 2^32)
    literal = np.array([_cmd(6, 0xFFFFFFFA, -3, 10), _cmd(9, 0, 5, 12), _cmd(3, 108, 0, 40), _cmd(12, 111, 7, 41), _cmd(6, 123, 7, 45)], DRAW_CMD_DTYPE)
    assert want.commands.tobytes() == literal.tobytes()
    assert (want.count, want.index_total, want.overflowed) == (5, 29, False)
    cut = mc.expected_merge([a, b, c], totals, 2)
    assert cut.commands.tobytes() == literal[:4].tobytes()
    assert (cut.count, cut.index_total, cut.overflowed) == (4, 29, True), "the index total is over the full header totals"
    one = mc.expected_merge([a, b, c], totals, 1)
    assert one.commands.tobytes() == literal[[0, 2]].tobytes() and one.overflowed and one.count == 2


@pytest.mark.parametrize("table_name", TABLES)
def test_expected_merge_is_the_oracles_merge(oracle_mod, table_name):
    for name in ENTRIES:
        lists, totals = mc.case(name, table_name)
        want = mc.expected_merge(lists, totals, mc.capacity_of(lists))
        merged, index_total = oracle_mod.merge_draw_lists([l.cmds for l in lists], totals)
        assert not want.overflowed and want.count == len(merged) == sum(mc.CATALOGUE[name]["counts"]), name
        assert want.commands.tobytes() == merged.tobytes() and want.index_total == index_total, name


# ---- the gloo test double ----

def _double_merge(tbl, buf, n_chunks, stride, capacity, form):
    pipe = OraclePipeline({"n": 1, "meshes": tbl})
    rows = n_chunks * capacity + mc.SLACK_ROWS
    out = np.full(rows * 5, mc.SENTINEL, np.uint32)
    count = np.full(2, mc.SENTINEL, np.uint32)
    buf = np.ascontiguousarray(buf)
    if form == "cmds":
        pipe.merge_draw_lists(buf.ctypes.data, n_chunks, stride, out.ctypes.data, count.ctypes.data, chunk_capacity=capacity)
    else:
        pipe.merge_wire_lists(buf.ctypes.data, n_chunks, stride, out.ctypes.data, count.ctypes.data, chunk_capacity=capacity, packed=form == "packed")
    return pipe, out, count


def _reports_overflow(pipe):
    from renderer_amd._lib import MipError

    try:
        pipe.wait()
    except MipError as e:
        assert e.code == -4
        return True
    return False


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("table_name", ["scene64", "t3", "t65"])
def test_the_test_double_merges_the_built_buffers(oracle_mod, table_name, form):
    tbl = mc.table(table_name)
    for name in ENTRIES:
        lists, totals = mc.case(name, table_name)
        cap = mc.capacity_of(lists)
        buf = mc.build_chunks(lists, totals, form, cap)
        pipe, out, count = _double_merge(tbl, buf, len(lists), mc.stride_for(cap, form), cap, form)
        mc.assert_merge(out, count, mc.expected_merge(lists, totals, cap), f"{name} {form}")
        assert not _reports_overflow(pipe), name


@pytest.mark.parametrize("position", ["alone", "middle"])
@pytest.mark.parametrize("which", ["minus1", "exact", "plus1", "ffffffff"])
@pytest.mark.parametrize("capacity", mc.CUT_CAPACITIES)
@pytest.mark.parametrize("form", mc.FORMS)
def test_the_test_double_cuts_at_the_capacity_and_reports_it(oracle_mod, form, capacity, which, position):
    lists, totals, header = mc.cut_case(capacity, which, position)
    buf = mc.build_chunks(lists, totals, form, capacity, header_counts=header)
    pipe, out, count = _double_merge(mc.table("scene64"), buf, len(lists), mc.stride_for(capacity, form), capacity, form)
    want = mc.expected_merge(lists, totals, capacity)
    assert want.overflowed == (which in ("plus1", "ffffffff")) and want.count == sum(min(len(l.cmds), capacity) for l in lists)
    mc.assert_merge(out, count, want, f"{form} capacity {capacity} {which} {position}")
    assert _reports_overflow(pipe) == want.overflowed


# ---- the comparison bites ----

def destination(commands, rows):
    out = np.full(rows * 5, mc.SENTINEL, np.uint32)
    out[:len(commands) * 5] = np.asarray(commands, DRAW_CMD_DTYPE).view(np.uint32).reshape(-1)
    return out


def test_the_gpu_tests_comparison_fails_on_wrong_merges():
    lists, totals = mc.case("align-255", "scene64")        # counts 255, 300, 7
    want = mc.expected_merge(lists, totals, 300)
    rows = 3 * 300 + mc.SLACK_ROWS
    right = want.commands
    mc.assert_merge(destination(right, rows), [want.count, want.index_total], want, "itself")
    # 1. the rebase of chunk 1 omitted
    wrong = right.copy()
    wrong["firstIndex"][255:555] -= np.uint32(totals[0])
    with pytest.raises(AssertionError, match="command 255 of 562"):
        mc.assert_merge(destination(wrong, rows), [want.count, want.index_total], want)
    # 2. the running sum of chunk 1's first sub-block carried into its second (which restarts at its own anchor)
    wrong = right.copy()
    wrong["firstIndex"][255 + 64:255 + 128] += np.uint32(int(right["indexCount"][255:255 + 64].astype(np.uint64).sum()) & mc.MASK)
    with pytest.raises(AssertionError, match="command 319 of 562"):
        mc.assert_merge(destination(wrong, rows), [want.count, want.index_total], want)
    # 3. one command behind the merged count overwritten
    out = destination(right, rows)
    out[want.count * 5:want.count * 5 + 5] = right[-1:].view(np.uint32).reshape(-1)
    with pytest.raises(AssertionError, match="behind the merged count"):
        mc.assert_merge(out, [want.count, want.index_total], want)
    out = destination(right, rows)
    out[-1] = 0
    with pytest.raises(AssertionError, match="behind the merged count"):
        mc.assert_merge(out, [want.count, want.index_total], want)
    # and the two scalars
    with pytest.raises(AssertionError, match="merged count"):
        mc.assert_merge(destination(right, rows), [want.count - 1, want.index_total], want)
    with pytest.raises(AssertionError, match="index total"):
        mc.assert_merge(destination(right, rows), [want.count, (want.index_total - totals[0]) & mc.MASK], want)
    with pytest.raises(AssertionError, match="no slack rows"):
        mc.assert_merge(destination(right, want.count + 1), [want.count, want.index_total], want)
