"""The hand-written slot orders of tests/order_cases.py against the restatement (tests/order_restatement.py), and the scenes
against their own documentation: every case's q has the bit pattern and K the module states."""
import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import order_cases as oc
import order_restatement as orr

F = np.float32
MODES = (lr.DISTANCE, lr.RELATIVE)
ORDERS = (orr.NEAR_FIRST, orr.FAR_FIRST)


def _q(pos):
    with np.errstate(all="ignore"):
        return (pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]


def test_the_edge_scene_is_what_its_table_says():
    s = oc.edge_scene()
    n = s["n"]
    q = _q(s["pos"])
    assert n == 1233 and n % 1024 != 0
    insts = [c[0] for c in oc.EDGE_CASES]
    assert insts[0] == n - 1 and {i % 64 for i in insts[1:]} == {0, 63}      # the ragged tile's last instance; lanes 0 and 63
    for inst, name, _, bits, k in oc.EDGE_CASES:
        if bits is None:
            assert np.isnan(q[inst]), name
        else:
            assert int(q[inst:inst + 1].view(np.uint32)[0]) == bits and bits >> 16 == k, (name, hex(int(q[inst:inst + 1].view(np.uint32)[0])))
        assert int(orr.k_of_q(q[inst:inst + 1])[0]) == k, name
        assert s["mesh_id"][inst] == 1
    assert int(q[319:320].view(np.uint32)[0]) == int(np.array([np.finfo(F).max]).view(np.uint32)[0])   # the largest finite float
    assert (s["mesh_id"] == 1).sum() == len(oc.EDGE_CASES) == len(oc.EDGE_NEAR_FIRST) == len(oc.EDGE_FAR_FIRST)
    assert sorted(oc.EDGE_NEAR_FIRST) == sorted(oc.EDGE_FAR_FIRST) == sorted(insts)
    # the pair with one K: different floats, the nearer one in the later tile
    assert q[1232] < q[64] and 1232 // 1024 == 1 and 64 // 1024 == 0
    # the hand orders are sorted by the documented K (a check of the table against itself, not of the restatement)
    k_of = {c[0]: c[4] for c in oc.EDGE_CASES}
    assert [k_of[i] for i in oc.EDGE_NEAR_FIRST] == sorted(k_of.values())
    assert [k_of[i] for i in oc.EDGE_FAR_FIRST] == sorted(k_of.values(), reverse=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
def test_hand_written_slot_orders_of_the_edge_scene(mode, order):
    s = oc.edge_scene()
    got = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], lc.all_bits(s["n"]), mode, lc.SWITCH, order,
                                  first_instance_base=5)
    want = oc.want_edge_slots(order == orr.NEAR_FIRST)
    assert got["members"] == s["n"] and got["count"] == 2 and not got["lod"].any()
    assert got["order"].tolist() == want.tolist()
    assert got["ids"].tolist() == (want + 5).tolist()
    assert got["cmds"]["instanceCount"].tolist() == [s["n"] - 13, 13] and got["cmds"]["firstInstance"].tolist() == [0, s["n"] - 13]


def test_the_tie_scene_is_what_its_comment_says():
    s = oc.tie_scene()
    g = oc.tie_groups()
    k = orr.k_of_q(_q(s["pos"]))
    assert np.array_equal(k, np.asarray(oc.TIE_K)[g])
    for edge in (64, 256, 1024, 2048):    # consecutive members of the x = 3 group on both sides of a round, a wave and two tiles
        assert (g[edge - 4:edge + 4] == 1).all()
    assert (g == 1).sum() > 1024 and (g == 0).sum() > 1000 and (g == 2).sum() > 1000


@pytest.mark.parametrize("order", ORDERS)
def test_hand_written_slot_orders_of_the_tie_scene(order):
    s = oc.tie_scene()
    got = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], lc.all_bits(s["n"]), lr.DISTANCE, lc.SWITCH, order)
    want = oc.want_tie_slots(order == orr.NEAR_FIRST)
    assert got["count"] == 1 and got["members"] == s["n"]
    assert got["order"].tolist() == want.tolist()


def test_the_digit_scene_is_what_its_table_says():
    s = oc.digit_scene()
    q = _q(s["pos"])
    assert s["n"] == 64 and len(s["meshes"]) == 1 and int(s["meshes"]["n_lods"][0]) == 2     # one round of one wave; the buckets are the LODs
    bits = q.view(np.uint32)
    cases = {c[0]: c for c in oc.DIGIT_CASES}
    for i in range(s["n"]):
        assert int(bits[i]) == (cases[i][2] if i in cases else oc.DIGIT_FILLER_BITS), i
    for mode in MODES:
        lod = lr.select_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], mode, lc.SWITCH)
        assert lod.tolist() == [cases[i][3] if i in cases else 0 for i in range(s["n"])], mode
    k = {i: c[2] >> 16 for i, c in cases.items()}
    flip = lambda v: 0x7F80 - v
    # one bucket, keys that differ only in the lowest digit ...
    assert cases[3][3] == cases[40][3] == 1 and k[3] >> 8 == k[40] >> 8 and k[3] & 255 != k[40] & 255
    assert flip(k[3]) >> 8 == flip(k[40]) >> 8 and flip(k[3]) & 255 != flip(k[40]) & 255
    # ... and a member of the other bucket with the lowest digit of one of them, near first and far first
    assert cases[7][3] == 0 and k[7] & 255 == k[40] & 255 and flip(k[7]) & 255 == flip(k[40]) & 255
    assert sorted(oc.DIGIT_NEAR_FIRST) == sorted(oc.DIGIT_FAR_FIRST) == list(range(64))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
def test_hand_written_slot_orders_of_the_digit_scene(mode, order):
    s = oc.digit_scene()
    got = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], lc.all_bits(s["n"]), mode, lc.SWITCH, order,
                                  first_instance_base=5)
    want = oc.want_digit_slots(order == orr.NEAR_FIRST)
    assert got["members"] == 64 and got["count"] == 2
    assert got["order"].tolist() == want.tolist()
    assert got["ids"].tolist() == (want + 5).tolist()
    assert got["cmds"]["instanceCount"].tolist() == list(oc.DIGIT_COUNTS) and got["cmds"]["firstInstance"].tolist() == [0, 62]
