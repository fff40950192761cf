"""tests/cluster_sequence_cases.py checked on the CPU: the scenes move every plan and leave no unit's expectation empty, the
sequences cover what they claim — every ordered pair of the eleven units, a larger and a smaller bound in front of every unit,
an overflow beside a fitting call of each status-word group, every refusal between two good calls — and each expectation mutant
(a stale input of the kind a shared scratch would supply) changes the expected bytes of at least one step of every unit it
applies to: the sequences can tell a stale read from a right one. The per-mutant, per-unit counts are printed (pytest -s)."""
import numpy as np
import pytest

import cluster_phase_restatement as pr
import cluster_sequence_cases as sq


def _calls(name, **kw):
    return [e for e in sq.expectations(sq.sequence(name), **kw) if e is not None and "unit" in e]


# ---- the scenes ----

def test_scene_sizes_move_every_plan():
    w = {name: {e["w"] for e in _calls("bounds_down_and_up") if e["scene"] == name} for name in sq.SCENE_NAMES}
    assert max(w["S"]) <= 1024, w["S"]                              # one item tile
    assert 1024 < min(w["M"]) and max(w["M"]) <= 16384, w["M"]      # several item tiles, one head tile and one list tile
    assert min(w["L"]) > 16384, w["L"]                              # two head tiles and two list tiles
    assert w["Z"] == {0}
    n = sq.n_of_l()
    assert sq._w_of(n) > 16384 >= sq._w_of(n - 1) and sq.max_instances() == n
    assert sq.scene("S")["max_clusters"] != sq.scene("M")["max_clusters"] and len(sq.scene("S")["s"]["meshes"]) != len(sq.scene("M")["s"]["meshes"])


@pytest.mark.parametrize("name", ["S", "M", "L"])
def test_no_unit_s_expectation_is_trivially_empty(name):
    """Per unit: a surviving cluster, a culled one and a member whose first item lies inside a 64-item word."""
    sc, seen = sq.scene(name), set()
    record = {}
    for unit in sq.UNITS:
        for bm in (0, 1):
            p = dict(sq.call(unit, rec="r" if unit in sq.FIRSTS + sq.SECONDS else None, bm=bm, pyramid=True, cone=True), room_bytes=None)
            if unit in sq.SECONDS:
                p["room_bytes"] = 4 * len(record[bm])
            a = sq.compute(sc, p, record=record.get(bm))
            if unit in sq.FIRSTS:
                record[bm] = a["record"]
            survive = a["survive"] if isinstance(a["survive"], list) else [a["survive"]]
            for v, sv in enumerate(survive):
                assert sv.any() and not sv.all(), (name, unit, bm, v)
            if unit in sq.SECONDS:      # of the recorded clusters some are visible under the new pyramid and some stay hidden
                bits = pr.unpack_record(record[bm], a["w"])
                assert (bits & survive[0]).any() and (bits & ~survive[0]).any(), (name, unit, bm)
            first_items = np.nonzero(a["items"]["cluster"] == 0)[0]
            assert (first_items % 64 != 0).any(), (name, unit, bm)
            assert a["status"] == sq.OK
            seen.add(unit)
    assert seen == set(sq.UNITS)


# ---- the sequences ----

def test_every_pair_is_adjacent_and_a_second_follows_its_first():
    units = [st["unit"] for st in sq.calls(sq.sequence("every_pair"))]
    pairs = set(zip(units, units[1:]))
    assert pairs >= {(a, b) for a in sq.UNITS for b in sq.UNITS} and len({(a, b) for a in sq.UNITS for b in sq.UNITS}) == 121
    for name in sq.SEQUENCES:           # expectations() finds every SECOND step's record among the FIRST steps since the last switch
        scene_now, first_of = None, {}
        for st in sq.sequence(name):
            if st["op"] == "scene":
                scene_now, first_of = st["scene"], {}
            elif st["op"] == "call" and st["unit"] in sq.FIRSTS and not st["refuse"]:
                first_of[st["rec"]] = st
            elif st["op"] == "call" and st["unit"] in sq.SECONDS:
                assert st["rec"] in first_of, (name, st)
    assert all(e["status"] == sq.OK for e in _calls("every_pair"))
    for field, values in (("async_", {False, True}), ("work", {"zero", "exact", "large"}), ("cap", {"room", "exact"}), ("n_views", {1, 3, 16})):
        for unit in sq.UNITS:
            got = {st[field] for st in sq.calls(sq.sequence("every_pair")) if st["unit"] == unit}
            assert got >= values, (unit, field, got)


def test_across_phases_puts_every_unit_between_a_first_and_its_second():
    steps = sq.calls(sq.sequence("across_phases"))
    for opener in sq.FIRSTS:
        closer = opener.replace("FIRST", "SECOND")
        between = set()
        for a, x, b in zip(steps, steps[1:], steps[2:]):
            if a["unit"] == opener and b["unit"] == closer and a["rec"] == b["rec"]:
                between.add(x["unit"])
        other = [f for f in sq.FIRSTS if f != opener][0]
        assert between >= set(sq.UNITS) - {other}, (opener, between)
        # the FIRST of the other entry point, with a record of its own: both SECOND calls in either order
        orders = set()
        for a, x, b, c in zip(steps, steps[1:], steps[2:], steps[3:]):
            if a["unit"] == opener and x["unit"] == other and {b["unit"], c["unit"]} == set(sq.SECONDS) and a["rec"] != x["rec"]:
                orders.add(b["rec"] == a["rec"])
        assert orders == {True, False}, opener
    assert all(e["status"] == sq.OK for e in _calls("across_phases"))


def test_bounds_go_down_and_up_in_front_of_every_unit():
    steps = sq.sequence("bounds_down_and_up")
    assert [st["scene"] for st in steps if st["op"] == "scene"] == list(sq.BOUNDS_ORDER) * 3
    calls = _calls("bounds_down_and_up")
    assert all(e["status"] == sq.OK for e in calls)
    visit = 2 * len(sq.UNITS)          # the steps of the present and of the previous visit
    for unit in sq.UNITS:
        larger = smaller = False
        for k, e in enumerate(calls):
            if e["unit"] != unit:
                continue
            others = [o for o in calls[max(k - visit, 0): k] if o["unit"] != unit]
            larger |= any(o["bound"] > e["bound"] for o in others)
            smaller |= any(o["bound"] < e["bound"] for o in others)
        assert larger and smaller, unit
    by_work = {w: {e["unit"] for e in calls if e["step"]["work"] == w} for w in ("zero", "exact", "large")}
    assert all(v == set(sq.UNITS) for v in by_work.values())
    for e in calls:                     # "exact" is exactly W, "large" is above every other bound of the context
        if e["step"]["work"] == "exact" and e["w"]:
            assert e["sizes"]["work"] == e["w"] == e["bound"] or e["unit"] in sq.FIRSTS + sq.SECONDS
        if e["step"]["work"] == "large":
            assert e["sizes"]["work"] > max(o["bound"] for o in calls if o["step"]["work"] != "large")


def test_overflow_isolation_pairs_every_unit_with_both_groups():
    steps = sq.sequence("overflow_isolation")
    ex = sq.expectations(steps)
    seen, mirrored = set(), set()
    k = 0
    while k < len(steps):
        if steps[k]["op"] == "call" and steps[k]["defer"]:
            x, y = ex[k], None
            j = k + 1
            while steps[j]["op"] == "call":
                y = ex[j]
                j += 1
            waits = []
            while j < len(steps) and steps[j]["op"] == "wait":
                waits.append(steps[j]["expect"])
                j += 1
            assert y["unit"] != x["unit"] and not y["step"]["async_"]
            if x["status"] == sq.CAPACITY:
                assert y["status"] == sq.OK and waits == [sq.CAPACITY, sq.OK], (k, x["unit"], y["unit"])
                seen.add((x["unit"], sq.group(y["unit"])))
            else:
                assert x["status"] == sq.OK and y["status"] == sq.CAPACITY and waits == [sq.OK], (k, x["unit"], y["unit"])
                mirrored.add((x["unit"], sq.group(y["unit"])))
            k = j
        else:
            k += 1
    every = {(u, g) for u in sq.UNITS for g in ("single-view", "several-view")}
    assert seen == every and mirrored == every
    kinds = {(e["step"]["work"] == "short", e["step"]["cap"] == "short") for e in ex if e is not None and e.get("status") == sq.CAPACITY and "unit" in e}
    assert kinds == {(True, False), (False, True)}


def test_refusals_sit_between_two_good_calls_of_other_kinds():
    steps = sq.sequence("refused_in_between")
    ex = sq.expectations(steps)
    kinds = set()
    calls = [(st, e) for st, e in zip(steps, ex) if st["op"] == "call"]
    for k, (st, e) in enumerate(calls):
        if e.get("refused"):
            assert e["status"] in (sq.NOT_READY, sq.INVALID)
            assert all((img == sq.SENTINEL).all() for name, img in e["images"].items() if name != "record" or st["unit"] in sq.FIRSTS)
            kinds.add((st["unit"], "stale" if e["status"] == sq.NOT_READY else st["refuse"]))
        elif e["status"] == sq.DEVICE:
            assert st["unit"] in sq.SECONDS and int(e["images"]["cmds" if st["unit"] == "phase.SECOND" else "entries"][0, 0]) == sq.SENTINEL
            kinds.add((st["unit"], "not its record"))
        else:
            assert e["status"] == sq.OK
            continue
        before = [c for c in calls[:k] if c[0]["unit"] not in (st["unit"], st["unit"].replace("SECOND", "FIRST"))][-1]
        after = calls[k + 1]
        assert before[1]["status"] == after[1]["status"] == sq.OK and len({before[0]["unit"], st["unit"], after[0]["unit"]}) == 3
    want = {(u, r) for u in sq.UNITS for r in ("stale", "misaligned")} | {(u, "views17") for u in sq.SEVERAL} | {(u, "not its record") for u in sq.SECONDS}
    assert kinds == want, kinds ^ want


def test_the_shortcut_changes_no_expectation():
    right = _calls("across_phases")
    saved = dict(sq._CACHE), dict(sq._FULL)
    sq._CACHE.clear(), sq._FULL.clear()
    sq.SHORTCUT = False
    try:
        long = _calls("across_phases")
    finally:
        sq.SHORTCUT = True
        sq._CACHE.clear(), sq._FULL.clear()
        sq._CACHE.update(saved[0]), sq._FULL.update(saved[1])
    assert len(right) == len(long) and not any(sq.differs(a, b) for a, b in zip(right, long))


# ---- the mutants ----

APPLIES = dict(stale_cones=("cull_cone", "tri_cone", "list"), stale_record=sq.SECONDS)


def test_every_mutant_changes_the_expected_bytes_of_every_unit_it_applies_to():
    counts = {m: dict.fromkeys(sq.UNITS, 0) for m in sq.MUTANTS}
    where = {m: {} for m in sq.MUTANTS}
    for name in sq.SEQUENCES:
        for frames in (1, 2):
            right = sq.expectations(sq.sequence(name), frames_in_flight=frames)
            for m in sq.MUTANTS:
                if frames == 1 and m != "other_slots_history":
                    continue
                wrong = sq.expectations(sq.sequence(name), mutant=m, frames_in_flight=frames)
                for k, (a, b) in enumerate(zip(right, wrong)):
                    if b is not None and b.get("applies") and sq.differs(a, b):
                        counts[m][b["unit"]] += 1
                        where[m].setdefault(b["unit"], f"{name}[{k}]")
    print("\nsteps whose expected bytes a mutant changes (the first one found)")
    for m in sq.MUTANTS:
        print(f"  {m:22s} " + "  ".join(f"{u}={counts[m][u]}" + (f" ({where[m][u]})" if u in where[m] else "") for u in APPLIES.get(m, sq.UNITS)))
    for m in sq.MUTANTS:
        for u in APPLIES.get(m, sq.UNITS):
            assert counts[m][u] > 0, (m, u)
