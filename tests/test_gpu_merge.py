"""The three merge kernels (mip_merge_draw_lists, mip_merge_wire_lists, mip_merge_wire_lists_packed) over synthetic shard
lists (tests/merge_cases.py): per-chunk counts at every sub-block, group and alignment edge, up to 64 chunks, the group-stride
loop forced and at the default grid, capacity cuts, corrupt words live and dead, argument edges, asynchronous calls. Every
chunk is built on the CPU with 0xDEADBEEF in each word the header leaves unspecified; the expectation is plain numpy."""
import numpy as np
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

OK, ERR_INVALID_ARGUMENT, ERR_CAPACITY, ERR_DEVICE = 0, -1, -4, -5
ENTRIES = list(mc.CATALOGUE)
TABLES = list(mc.TABLE_SIZES)


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()  # fails loudly if the HIP library is missing
    return renderer_amd


@pytest.fixture(scope="module")
def contexts(ra):
    """One small context per mesh table, for the whole module."""
    made = {}

    def get(table_name):
        if table_name not in made:
            p = ra.InstancePipeline(max_instances=1, max_meshes=mc.TABLE_SIZES[table_name])
            p.set_mesh_table(mc.table(table_name))
            made[table_name] = p
        return made[table_name]

    yield get
    for p in made.values():
        p.close()


def _i32(words):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32))


def run_merge(ra, p, buf, n_chunks, stride, capacity, form, rows=None, offset_words=0, async_=False, chunks_offset_bytes=0):
    """Uploads the receive buffer, fills the destination (rows + 64 slack rows) and out_count with the sentinel, merges.
    Returns (status, destination words, out_count words); the destination starts offset_words words behind a 256-byte aligned
    address."""
    import torch

    dev = torch.device("cuda", 0)
    rows = n_chunks * capacity if rows is None else rows
    pad = chunks_offset_bytes // 4
    chunks = torch.empty(len(buf) + pad, dtype=torch.int32, device=dev)
    chunks[pad:] = _i32(buf).to(dev)
    fill = int(np.uint32(mc.SENTINEL).view(np.int32))
    out = torch.full(((rows + mc.SLACK_ROWS) * 5 + 4,), fill, dtype=torch.int32, device=dev)
    count = torch.full((2,), fill, dtype=torch.int32, device=dev)
    assert out.data_ptr() % 256 == 0 and chunks.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    status = OK
    try:
        args = (chunks.data_ptr() + chunks_offset_bytes, n_chunks, stride, out.data_ptr() + 4 * offset_words, count.data_ptr())
        if form == "cmds":
            p.merge_draw_lists(*args, async_=async_, chunk_capacity=capacity)
        else:
            p.merge_wire_lists(*args, async_=async_, chunk_capacity=capacity, packed=form == "packed")
        if async_:
            p.wait()
    except ra.MipError as e:
        status = e.code
    torch.cuda.synchronize()
    words = out.cpu().numpy().view(np.uint32)
    assert np.all(words[:offset_words] == mc.SENTINEL), "words in front of the destination were written"
    return status, words[offset_words:offset_words + (rows + mc.SLACK_ROWS) * 5], count.cpu().numpy().view(np.uint32)


def check(ra, p, lists, totals, form, capacity, what, status=None, header_counts=None, **kw):
    want = mc.expected_merge(lists, totals, capacity)
    buf = mc.build_chunks(lists, totals, form, capacity, header_counts=header_counts)
    got_status, out, count = run_merge(ra, p, buf, len(lists), mc.stride_for(capacity, form), capacity, form, **kw)
    mc.assert_merge(out, count, want, what)
    assert got_status == ((ERR_CAPACITY if want.overflowed else OK) if status is None else status), f"{what}: status {got_status}"
    return want


# ---- the whole catalogue ----

@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("table_name", TABLES)
@pytest.mark.parametrize("form", mc.FORMS)
def test_catalogue(ra, contexts, form, table_name, name):
    lists, totals = mc.case(name, table_name)
    check(ra, contexts(table_name), lists, totals, form, mc.capacity_of(lists), f"{name} {table_name} {form}")


@pytest.mark.parametrize("offset_bytes", [4, 8, 12])
@pytest.mark.parametrize("c0", mc.ALIGN_C0)
@pytest.mark.parametrize("form", mc.FORMS)
def test_destination_that_is_only_four_byte_aligned(ra, contexts, form, c0, offset_bytes):
    lists, totals = mc.case(f"align-{c0}", "scene64")
    check(ra, contexts("scene64"), lists, totals, form, 300, f"align-{c0} +{offset_bytes} B {form}", offset_words=offset_bytes // 4)


# ---- the group-stride loop ----

def _stride_loop_case(shape):
    tbl = mc.table("scene64")
    if shape == "8x5000":
        counts = [5600, 5599, 5601, 4097, 0, 5603, 5376, 5377]
    else:
        rng = np.random.default_rng(64)
        counts = [int(c) for c in rng.integers(0, 2000, 64)]
        counts[5] = counts[40] = 0
        counts[63] = 1999
    lists = mc.make_lists(tbl, counts, 0x5712DE + len(counts))
    return lists, [l.total for l in lists]


@pytest.mark.parametrize("grid", [1, 3, 17])
@pytest.mark.parametrize("shape", ["8x5000", "64ragged"])
@pytest.mark.parametrize("form", ["wire", "packed"])
def test_stride_loop_forced_by_a_small_grid(ra, contexts, monkeypatch, form, shape, grid):
    """MIP_TUNE_MERGE_GRID caps the wire merge's grid (read at every call): with 1, 3 or 17 workgroups every wave walks many
    groups of many chunks, re-using its staging area each time."""
    lists, totals = _stride_loop_case(shape)
    capacity = mc.capacity_of(lists)
    groups = sum((len(l.cmds) + 255) // 256 for l in lists)
    assert groups > 2 * 4 * grid, "the capped grid has less than half as many waves as there are groups"
    monkeypatch.setenv("MIP_TUNE_MERGE_GRID", str(grid))
    check(ra, contexts("scene64"), lists, totals, form, capacity, f"{shape} grid {grid} {form}")


@pytest.mark.parametrize("form", ["packed", "wire"])
def test_stride_loop_at_the_default_grid_config4_shape(ra, contexts, monkeypatch, form):
    """BASELINE configs[3] as eight ranks exchange it: about 337 k commands per shard in chunks of 400 k, more groups than the
    default grid has waves, so waves take a second group with no tuning variable set."""
    monkeypatch.delenv("MIP_TUNE_MERGE_GRID", raising=False)
    n_chunks, capacity = 8, 400_000
    grid_cap = 256 * 8   # enqueue_merge_wire (renderer_amd/csrc/api_sharded.hip): `256u * 8u` workgroups of four waves, one group per wave and step
    assert -(-capacity // 256) * n_chunks > 4 * grid_cap
    counts = [337_000, 336_911, 337_409, 335_872, 337_153, 338_001, 336_640, 337_215]
    assert sum(-(-c // 256) for c in counts) > 4 * grid_cap, "also by the groups that exist"
    lists = mc.make_lists(mc.table("scene64"), counts, 0xC0F164)
    check(ra, contexts("scene64"), lists, [l.total for l in lists], form, capacity, f"config 4 shape {form}")


# ---- capacity cuts ----

@pytest.mark.parametrize("position", ["alone", "middle"])
@pytest.mark.parametrize("which", ["minus1", "exact", "plus1", "ffffffff"])
@pytest.mark.parametrize("capacity", mc.CUT_CAPACITIES)
@pytest.mark.parametrize("form", mc.FORMS)
def test_capacity_cut(ra, contexts, form, capacity, which, position):
    """A chunk whose header count exceeds the capacity is cut there and reported — also at wire capacities that are not whole
    sub-blocks, and for a header of 0xFFFFFFFF: all three kernels clamp the count to the capacity before its first use
    (merge_kernel.hpp: `count = capacity` in the table loop; `t_count = t_count > capacity ? capacity : t_count` ahead of the
    scans), so that case is a documented status like the others."""
    lists, totals, header = mc.cut_case(capacity, which, position)
    want = check(ra, contexts("scene64"), lists, totals, form, capacity, f"{form} capacity {capacity} {which} {position}", header_counts=header)
    assert want.overflowed == (which in ("plus1", "ffffffff"))
    assert want.count == sum(min(len(l.cmds), capacity) for l in lists)
    if want.overflowed:  # the same context merges a clean buffer next
        clean, clean_totals = mc.case("align-3", "scene64")
        check(ra, contexts("scene64"), clean, clean_totals, form, 300, "clean after an overflow")


# ---- corrupt words, live and dead ----

CORRUPT_TABLE = "t65"   # 65 entries: seven mesh bits in a packed record, so it can name meshes 65..127, which do not exist


def _corrupt_case():
    """Chunk 1 ends in a partial sub-block: 150 records = two whole sub-blocks and 22 records of a third."""
    lists = mc.make_lists(mc.table(CORRUPT_TABLE), [70, 150, 9], 0xBAD)
    return lists, [l.total for l in lists]


def _record_word(form, stride, chunk, record):
    """Index (in the receive buffer's words) of the word of `record` that carries the mesh id."""
    base = chunk * stride // 4 + mc.HEADER_WORDS
    if form == "wire":
        return base + record // 256 * 516 + 4 + 2 * (record % 256) + 1
    return base + record // 64 * 68 + 4 + record % 64


@pytest.mark.parametrize("form", ["wire", "packed"])
def test_corrupt_mesh_id_live_and_dead(ra, contexts, form):
    p = contexts(CORRUPT_TABLE)
    tbl = mc.table(CORRUPT_TABLE)
    lists, totals = _corrupt_case()
    capacity, stride = 150, mc.stride_for(150, form)
    want = mc.expected_merge(lists, totals, capacity)
    bits = mc.wire_index_bits(len(tbl))
    for record, status in ((149, ERR_DEVICE), (150, OK)):   # the last live record of the partial sub-block, the first dead slot behind it
        buf = mc.build_chunks(lists, totals, form, capacity)
        w = _record_word(form, stride, 1, record)
        if form == "wire":
            buf[w] = len(tbl)                                            # mesh 65 of a 65-entry table, lod 0
        else:
            index = int(buf[w]) & ((1 << bits) - 1) if record == 149 else 5
            buf[w] = index | (127 << bits)                               # mesh 127, lod 0
        ref = want
        if status != OK:   # that record is expanded as mesh 0, lod 0: its own indexCount and vertexOffset change, and the firstIndex of nothing (it is the last of its sub-block)
            cmds = want.commands.copy()
            assert tbl["index_len"][0, 0] != cmds["indexCount"][70 + 149] or tbl["vertex_offset"][0] != cmds["vertexOffset"][70 + 149]
            cmds["indexCount"][70 + 149] = tbl["index_len"][0, 0]
            cmds["vertexOffset"][70 + 149] = tbl["vertex_offset"][0]
            ref = want._replace(commands=cmds)
        got, out, count = run_merge(ra, p, buf, 3, stride, capacity, form)
        mc.assert_merge(out, count, ref, f"{form} record {record}")
        assert got == status, (form, record, got)
        check(ra, p, lists, totals, form, capacity, "clean after a corrupt record")


def test_corrupt_packed_block_header_live_and_dead(ra, contexts):
    p = contexts("scene64")
    lists = mc.make_lists(mc.table("scene64"), [70, 128, 9], 0xB175)   # chunk 1: exactly two blocks; a third fits the stride
    totals = [l.total for l in lists]
    capacity, stride = 192, mc.stride_for(192, "packed")
    want = mc.expected_merge(lists, totals, capacity)
    for block, status in ((1, ERR_DEVICE), (2, OK)):   # the last existing block, the block behind the count
        buf = mc.build_chunks(lists, totals, "packed", capacity)
        buf[stride // 4 + mc.HEADER_WORDS + 68 * block + 2] = 40   # index_bits = 40
        got, out, count = run_merge(ra, p, buf, 3, stride, capacity, "packed")
        assert got == status, (block, got)
        assert int(count[0]) == want.count and int(count[1]) == want.index_total
        if status == OK:
            mc.assert_merge(out, count, want, "corrupt header behind the count")
        else:  # every command outside that block is as expected, and nothing lands behind the list
            rows = out[:want.count * 5].reshape(-1, 5)
            ref = want.commands.view(np.uint32).reshape(-1, 5)
            keep = np.ones(want.count, bool)
            keep[70 + 64:70 + 128] = False
            assert np.array_equal(rows[keep], ref[keep]) and np.all(out[want.count * 5:] == mc.SENTINEL)
        check(ra, p, lists, totals, "packed", capacity, "clean after a corrupt header")


# ---- argument edges ----

@pytest.mark.parametrize("form", mc.FORMS)
def test_argument_edges(ra, contexts, form):
    p = contexts("scene64")
    lists, totals = mc.case("chunks-64", "scene64")
    capacity = mc.capacity_of(lists)
    stride = mc.stride_for(capacity, form)
    buf = mc.build_chunks(lists, totals, form, capacity)

    def refused(what, n_chunks=64, stride=stride, capacity=capacity, chunks_offset_bytes=0):
        status, out, count = run_merge(ra, p, buf, n_chunks, stride, capacity, form, rows=64, chunks_offset_bytes=chunks_offset_bytes)
        assert status == ERR_INVALID_ARGUMENT, (what, status)
        assert np.all(out == mc.SENTINEL) and np.all(count == mc.SENTINEL), f"{what}: nothing is written"

    refused("no chunks", n_chunks=0)
    refused("65 chunks", n_chunks=65)
    refused("a stride that does not hold the capacity", stride=stride - 256)
    refused("a stride below the header", stride=16, capacity=0)
    if form != "cmds":
        refused("wire chunks that are not 16-byte aligned", chunks_offset_bytes=8)
        refused("a wire stride that is not 16-byte aligned", stride=stride + 8)
    else:
        refused("a stride that is not a multiple of 4", stride=stride + 2)
    # 64 chunks are merged
    check(ra, p, lists, totals, form, capacity, "64 chunks")
    # chunk_capacity = 0: what the stride holds (whole blocks for the wire forms)
    holds = {"cmds": (stride - 32) // 20, "wire": (stride - 32) // 2064 * 256, "packed": (stride - 32) // 272 * 64}[form]
    assert holds >= capacity
    status, out, count = run_merge(ra, p, buf, 64, stride, 0, form, rows=64 * capacity)
    mc.assert_merge(out, count, mc.expected_merge(lists, totals, holds), f"{form} capacity 0")
    assert status == OK
    # ... and a count above it is cut there
    big = mc.make_lists(mc.table("scene64"), [holds + 1, 3], 0xCA9)
    cut = mc.expected_merge(big, [l.total for l in big], holds)
    status, out, count = run_merge(ra, p, mc.build_chunks(big, [l.total for l in big], form, capacity, stride=stride), 2, stride, 0, form, rows=2 * holds)
    mc.assert_merge(out, count, cut, f"{form} capacity 0, count above what the stride holds")
    assert status == ERR_CAPACITY and cut.count == holds + 3


# ---- asynchronous calls ----

@pytest.mark.parametrize("form", mc.FORMS)
def test_async_status_arrives_from_wait_and_timing_counts_synchronous_merges(ra, form):
    tbl = mc.table(CORRUPT_TABLE)
    lists = mc.make_lists(tbl, [40, 0, 257, 258, 17, 257], 0xA57C)
    totals, header = [l.total for l in lists], None
    clean, clean_totals = mc.case("align-3", CORRUPT_TABLE)
    with ra.InstancePipeline(max_instances=1, max_meshes=len(tbl), timing=True) as p:
        p.set_mesh_table(tbl)
        p.reset_timings()
        check(ra, p, clean, clean_totals, form, 300, "synchronous")
        assert p.timings()["merges"] == 1
        check(ra, p, clean, clean_totals, form, 300, "asynchronous", async_=True)
        assert p.timings()["merges"] == 1, "only synchronous merges are timed"
        # the overflow of an asynchronous merge is reported by wait(), not by the call
        import torch

        dev = torch.device("cuda", 0)
        buf = mc.build_chunks(lists, totals, form, 257, header_counts=header)
        chunks = _i32(buf).to(dev)
        out = torch.zeros((6 * 257 + 64) * 5, dtype=torch.int32, device=dev)
        count = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        args = (chunks.data_ptr(), 6, mc.stride_for(257, form), out.data_ptr(), count.data_ptr())
        if form == "cmds":
            p.merge_draw_lists(*args, async_=True, chunk_capacity=257)
        else:
            p.merge_wire_lists(*args, async_=True, chunk_capacity=257, packed=form == "packed")
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == ERR_CAPACITY
        p.wait()   # reported once
        check(ra, p, lists, totals, form, 257, "the same cut through run_merge, asynchronous", header_counts=header, async_=True)
        if form != "cmds":   # a corrupt record of an asynchronous merge: MIP_ERR_DEVICE from wait()
            bad = mc.build_chunks(clean, clean_totals, form, 300)
            bad[_record_word(form, mc.stride_for(300, form), 1, 0)] = len(tbl) if form == "wire" else 127 << mc.wire_index_bits(len(tbl))
            status, _, count = run_merge(ra, p, bad, 3, mc.stride_for(300, form), 300, form, async_=True)
            assert status == ERR_DEVICE and int(count[0]) == 310
        check(ra, p, clean, clean_totals, form, 300, "clean after the errors")
        assert p.timings()["merges"] == 2
