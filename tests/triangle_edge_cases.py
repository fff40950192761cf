"""Decision-edge triangles for the per-triangle test (generate_work.comp:137-166; renderer_amd/csrc/triangle_kernels.hpp,
triangle_cull_clip), written in CLIP space with hand-stated answers. Pure numpy, no GPU.

A case is three corners (x, y, w) as float32 bit patterns, a hand-stated `kept`, one line of why, and the group it belongs to.
A group is a pv matrix and an instance transform. Every pv has only +-0, +-1 or +-4 as entries, and every instance a scale and
a translation that are powers of two, so the builder can realise a clip corner as a mesh vertex whose clip coordinates under
the float32 chain  pv * (model * vec4(v, 1))  are the intended bits (tests/test_triangle_edge_cases.py checks every corner).

The pv matrices. Every zero entry is -0 and the w row is (-0, -0, -p, -0), because that is the only way to reach w = -0:
    clip.w = ((-0 * wx + -0 * wy) + -p * wz) + -0 * 1
is -0 exactly when wz = +0 and both wx >= 0 and wy >= 0 (every term is then -0); one negative wx or wy makes its product +0
and the sum +0. (With +0 entries w = -0 is unreachable: (+0 + -0) = +0.) So
    "pos"       x row (1, -0, -0, -0), y row (-0, 1, -0, -0):  clip = (vx, vy, -vz);   w = -0 needs x, y >= 0
    "neg"       x row (-1, ...),       y row (.., -1, ..):     clip = (-vx, -vy, -vz); w = -0 needs x, y <= 0
    "overflow"  x and y rows 4, w row -4:                      clip = (4 vx, 4 vy, -4 vz): 4 * 2^127 = inf, the only way to an
                                                               infinite clip value beside finite ones (an infinite VERTEX
                                                               coordinate turns every 0 * inf of the chain into NaN)
The z row is (-0, -0, 1, -0): clip.z = wz = -clip.w / p, so a determinant taken over xyz has the other sign than over xyw.
A world coordinate that is zero is always +0 (world.x = ((1 * x + 0 * y) + 0 * z) + 0 ends in "+ +0"), which is why the sign of
a zero w follows the signs of x and y, and why the sign of a zero x or y is not the case's to choose: the catalogue pins the
bits of every w, and of every x and y except the sign of a zero. No decision depends on that sign: +-0 compare equal, a
quotient +-0 / w is +-0 or NaN either way, and a product that is +-0 adds nothing to a determinant that is compared with > 0.

The groups: "pos", "neg", "overflow" under the identity instance (pos 0, rot (0,0,0,1), scale 1: the model matrix is exactly
the identity); "scaled" = pv "pos" under scale 2 and translation +-2^-10 (world = 2 v + t, exact for the cases listed there);
"mirror" = pv "pos" under triangle_cases.MIRROR_INSTANCE (world = (x, 2 - y, z), a matrix with -0 entries and scale -1).
Every vertex of every mesh is FINITE, so that the library may choose the affine chain (triangle_test<true>); a NaN corner is
reached by overflow under "scaled" (_nan_cases), an infinite one under "overflow" (_infinite_cases).

Which cases run under "scaled" and "mirror". A translation t makes  s v + t  exact only where the clip value c and c - t fit one
significand: with t = 2^-10 that is |c| within about [2^-25, 2), with t = 2 (mirror, y only) it is c in about (-2, 4) at a
spacing of 2^-22 or coarser. So these never realise there, by arithmetic and not by choice: the subnormal class and
det = +-2^-149 (c - t rounds c away), the exponent families 2^-126, 2^-40, 2^40, 2^127, the all-ones mantissa 2 - 2^-23 under
"scaled" (its corner 4 - 2^-22 plus 2^-10 needs 26 bits) and the `wstar` family (a 24-bit mantissa next to 2^-10); under
"mirror" also the y families on the negative side (2 + 1 + 2^-23 needs 25 bits). What remains is flagged per case (model=,
mirror=): the b = 1 NDC family in all four kinds on both axes, sides and signs of w, the mixed-sign and zero-w cases, every
determinant case but +-2^-149, and (scaled) the NaN corners. test_every_case_is_realised_bit_for_bit fails on a wrong flag.

Not covered: a determinant whose sign differs under an expansion along another row. The issue lists it as an alternative to
the reassociation t0 - (t1 - t2), which is covered (det_association_*, mutant det_reassociated).

Determinant. det = (x0 (y1 w2 - y2 w1) - x1 (y0 w2 - y2 w0)) + x2 (y0 w1 - y1 w0), one rounding per operation, culled when
det > 0. The NDC families below are built so that the determinant is decided on paper:
    corners  (t_k, o_k, w_k)  with  w = sg (b, b, 2b),  o = (o0, o1, o2) b,  t = the tested coordinate (x, or y with the
    roles of x and y exchanged, which changes the determinant's sign).
  * t_k = c w_k (on the bound c = 1; beyond it by one ulp, since nextafter(2b) = 2 nextafter(b)): the t column is a multiple of
    the w column, every cofactor product is a power-of-two multiple of the same two mantissas, the three terms cancel bit
    for bit: det = +-0, the NDC test alone decides. Where the products overflow (b = 2^127) det is NaN, where they underflow
    (b <= 2^-124) it is 0: not > 0 either.
  * two corners beyond, the third on (b a power of two: every operation exact): det = -+ b^2 (a - b) / 2, the sign chosen by
    the order of o0, o1.
  * one corner beyond the OTHER bound: a triangle three units wide, |det| ~ 3 b^3, its sign chosen by o.
"""
import numpy as np

import triangle_cases as tc

F = np.float32
U32 = np.uint32
SENTINEL = 0xFFFFFFFF
NAN = F(np.nan)
INF = F(np.inf)
TINY = F(2.0 ** -149)                   # the smallest subnormal
NORMAL_MIN = F(2.0 ** -126)
WSTAR = np.array([0x3F9E48B3], U32).view(F)[0]   # 1.2365936: nextafter(w) * RN(1 / w) == 1 although nextafter(w) / w > 1


def bits(x):
    return np.ascontiguousarray(x, F).view(U32)


def up(x, k=1):
    """x moved k floats away from zero (k < 0: towards it)."""
    x = F(x)
    away = F(np.copysign(np.inf, x)) if k > 0 else F(0)
    for _ in range(abs(k)):
        x = np.nextafter(x, away)
    return F(x)


def _pv(px, py, pw):
    m = np.full(16, -0.0, F)            # column-major: m[c * 4 + r]
    m[0 * 4 + 0], m[1 * 4 + 1], m[2 * 4 + 2], m[2 * 4 + 3] = px, py, 1.0, -pw
    return m


PVS = {"pos": _pv(1, 1, 1), "neg": _pv(-1, -1, 1), "overflow": _pv(4, 4, 4)}
IDENTITY_INSTANCE = dict(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0), scale=1.0)
SCALED_INSTANCE = dict(pos=(2.0 ** -10, -(2.0 ** -10), 2.0 ** -10), rot=(0.0, 0.0, 0.0, 1.0), scale=2.0)
# unit: the smallest clip step the group can realise; e_min: the smallest exponent at which a corner one ulp off is realisable
GROUPS = {
    "pos": dict(pv="pos", instance=IDENTITY_INSTANCE, unit=TINY, e_min=-126, full=True),
    "neg": dict(pv="neg", instance=IDENTITY_INSTANCE, unit=TINY, e_min=-126, full=True),
    "overflow": dict(pv="overflow", instance=IDENTITY_INSTANCE, unit=F(4) * TINY, e_min=-124, full=True),
    "scaled": dict(pv="pos", instance=SCALED_INSTANCE, full=False),
    "mirror": dict(pv="pos", instance=tc.MIRROR_INSTANCE, full=False),
}
PV_OF = {g: d["pv"] for g, d in GROUPS.items()}


class Case:
    def __init__(self, name, cls, corners, kept, why, model=False, mirror=False):
        self.name, self.cls, self.kept, self.why, self.model, self.mirror = name, cls, bool(kept), why, model, mirror
        self.clip = np.array(corners, F).reshape(3, 3)           # rows: corners; columns: x, y, w
        self.bits = bits(self.clip).copy()

    def __repr__(self):
        return f"Case({self.name})"


# ---- the families ---------------------------------------------------------------------------------------------------------

def _corners(axis, t, o, w):
    """Corners from the tested coordinate t, the other coordinate o and w (three each)."""
    return [(t[k], o[k], w[k]) if axis == "x" else (o[k], t[k], w[k]) for k in range(3)]


def _ndc_cases(g):
    """The NDC bound, on x and y, both sides s, w > 0 and w < 0 (sg): q = t / w is beyond side s when t sg s > |w|."""
    out = []
    for axis in "xy":
        for s in (1, -1):
            for sg in (1, -1):
                tag = f"{axis}{'+' if s > 0 else '-'}_w{'pos' if sg > 0 else 'neg'}"
                first_big = (s > 0) == (axis == "x")              # which order of o makes det < 0 (module docstring)

                def family(b, kinds, label, grow=F(2), model=False, mirror=False):
                    b = F(b)
                    e = F(2.0) ** np.floor(np.log2(np.float64(b))).astype(F)  # o is scaled by b's power of two: |o| <= |w|
                    wa = [b, b, F(b * grow)]                                    # |w|
                    w = [F(sg) * v for v in wa]
                    sign = F(sg * s)
                    for kind in kinds:
                        mir = mirror and (axis == "x" or sg * s > 0)            # 2 - y is exact for these
                        if kind == "on":
                            t, o = [sign * v for v in wa], [F(0.25) * e, F(0.5) * e, e * min(grow, F(1))]
                            out.append(Case(f"ndc_{tag}_{label}_all_on", "ndc", _corners(axis, t, o, w), True,
                                            "t == w sg s for all three: on the bound, not beyond; t column = +-w column: det = +-0 or NaN", model, mir))
                        elif kind == "beyond":
                            t, o = [sign * up(v) for v in wa], [F(0.25) * e, F(0.5) * e, e * min(grow, F(1))]
                            out.append(Case(f"ndc_{tag}_{label}_all_beyond", "ndc", _corners(axis, t, o, w), False,
                                            "all three one ulp beyond the same bound", model, mir))
                        elif kind == "two_beyond":
                            t = [sign * up(wa[0]), sign * up(wa[1]), sign * wa[2]]
                            o = [F(0.5) * e, F(0.25) * e, e] if first_big else [F(0.25) * e, F(0.5) * e, e]
                            out.append(Case(f"ndc_{tag}_{label}_two_beyond_one_on", "ndc", _corners(axis, t, o, w), True,
                                            "the third corner is ON the bound; det = -b^2 (a - b) / 2 < 0, every operation exact", model, mir))
                        elif kind == "split":
                            t = [-sign * up(wa[0]), sign * up(wa[1]), sign * up(wa[2])]
                            o = [F(0.25) * e, e, F(0.5) * e] if first_big else [F(0.5) * e, F(0.25) * e, e]
                            out.append(Case(f"ndc_{tag}_{label}_one_beyond_the_other_bound", "ndc", _corners(axis, t, o, w), True,
                                            "corner 0 beyond the opposite bound, two beyond this one: no bound has all three; det ~ -3 b^3", model, mirror and axis == "x"))

                family(1.0, ("on", "beyond", "two_beyond", "split"), "1", model=True, mirror=True)
                family(up(F(2.0), -1), ("on", "beyond"), "mantissa_ones", mirror=True)  # nextafter crosses the binade (2 v + t is not exact here)
                family(WSTAR, ("on", "beyond"), "wstar")                                   # beyond, but t * (1 / w) == 1
                family(F(2.0) ** F(g["e_min"]), ("on", "beyond"), "smallest_normal")
                family(F(2.0 ** -40), ("on", "beyond"), "2^-40")
                family(F(2.0 ** 40), ("on", "beyond"), "2^40")
                family(F(2.0 ** 127), ("on", "beyond"), "largest_exponent", grow=F(0.5))
    return out


def _subnormal_cases(g):
    """w = +-unit and the largest subnormal (of the group's unit), the tested coordinate on either side of it."""
    u = F(g["unit"])
    big = F(NORMAL_MIN - u)
    out = []
    for axis in "xy":
        for s in (1, -1):
            for sg in (1, -1):
                tag = f"{axis}{'+' if s > 0 else '-'}_w{'pos' if sg > 0 else 'neg'}"
                sign = F(sg * s)
                for label, wa, ta, kept, why in (
                        ("smallest_beyond", u, F(2) * u, False, "t / w = 2 for all three (a flushed w would give 0 / 0: kept)"),
                        ("smallest_on", u, u, True, "t / w = 1: on the bound; every product underflows: det = 0"),
                        ("largest_beyond", big, NORMAL_MIN, False, "t is the smallest normal, one step beyond the largest subnormal w"),
                        ("largest_on", big, big, True, "t == w sg s: on the bound"),
                        ("largest_inside", big, F(big - u), True, "one step inside")):
                    t, w, o = [sign * ta] * 3, [F(sg) * wa] * 3, [u, -u, u]
                    out.append(Case(f"sub_{tag}_{label}", "ndc", _corners(axis, t, o, w), kept, why))
    return out


def _zero_w_cases(g):
    """w = +-0. q: the quadrant in which this pv gives w = -0 (x q >= 0 and y q >= 0); one coordinate of the other sign gives +0."""
    q = F(-1.0 if g["pv"] == "neg" else 1.0)
    nz, pz = F(-0.0), F(0.0)
    zero = F(0.0)
    out = [
        Case("zero_w_all_negative_zero", "ndc", [(q * 1, q * 1, nz), (q * 2, q * 3, nz), (q * 0.5, q * 4, nz)], False,
             "x / -0 = -q inf for all three: beyond one bound"),
        Case("zero_w_all_positive_zero", "ndc", [(-q * 1, q * 1, pz), (-q * 2, q * 3, pz), (-q * 0.5, q * 4, pz)], False,
             "x / +0 = -q inf for all three"),
        Case("zero_w_both_zeros_no_common_bound", "ndc", [(q * 1, q * 1, nz), (-q * 1, q * 1, pz), (q * 1, -q * 1, pz)], True,
             "x / w = -q inf, -q inf, +q inf and y / w = -q inf, +q inf, -q inf: no bound has all three; every product is +-0: det = +-0"),
        Case("zero_w_sign_bit_decides_culled", "ndc", [(q * 2, q * 1, nz), (-q * 5, q * 0.25, 2), (-q * 3, q * 0.5, 1)], False,
             "corner 0: x / -0 = -q inf, the side of the other two (x / w = -2.5 q, -3 q): culled. Taken by `w < 0` corner 0 is on the "
             "other side and the triangle survives (det = -2.5)"),
        Case("zero_w_sign_bit_decides_kept", "ndc", [(q * 2, q * 1, nz), (q * 5, q * 0.25, 2), (q * 3, q * 0.5, 1)], True,
             "corner 0: x / -0 = -q inf, the others +2.5 q, +3 q: no common bound, det = -0.5. Taken by `w < 0` all three are beyond +q"),
        Case("zero_over_negative_zero", "ndc", [(zero, q * 1, nz), (zero, q * 2, nz), (q * 1, q * 1, 1)], True,
             "x / w = 0 / 0 = NaN for two corners: no x bound; y / w = -q inf, -q inf, q: no y bound; det = x2 (y0 w1 - y1 w0) = +-0"),
        Case("zero_over_positive_zero", "ndc", [(zero, -q * 1, pz), (zero, -q * 2, pz), (q * 1, q * 1, 1)], True,
             "0 / +0 = NaN; y / w = -q inf, -q inf, q; det = +-0"),
    ]
    # the same on the y bounds: x and y exchanged in every corner (w = -0 needs both of one sign, so the quadrant rule holds), and
    # corners 1 and 2 exchanged, which undoes the change of the determinant's sign
    twins = []
    for c in out[3:]:
        k = c.clip
        corners = [(k[0, 1], k[0, 0], k[0, 2]), (k[2, 1], k[2, 0], k[2, 2]), (k[1, 1], k[1, 0], k[1, 2])]
        twins.append(Case(c.name + "_on_y", "ndc", corners, c.kept, "x and y exchanged, corners 1 and 2 exchanged: " + c.why.replace("x /", "y /")))
    return out + twins


def _mixed_w_cases():
    return [
        Case("mixed_w_signs_x", "ndc", [(5, 0.25, 2), (-3, 0.5, -1), (3, 0.5, 1)], False,
             "x / w = 2.5, 3, 3: all beyond the right bound (det = -1). Without the sign flip corner 1 is on the left", model=True, mirror=True),
        Case("mixed_w_signs_y", "ndc", [(0.5, 3, 1), (0.5, -3, -1), (0.25, 5, 2)], False,
             "y / w = 3, 3, 2.5: all beyond the upper bound (det = -1)", model=True),
    ]


def _det_cases(g):
    a, b2 = F(1 + 2.0 ** -12), F(1 + 2.0 ** -11)   # a * a = 1 + 2^-11 + 2^-24 rounds (to even) to b2; fma(a, a, -b2) = 2^-24
    u = F(g.get("unit", TINY))
    out = [
        Case("det_two_equal_corners", "det", [(0.25, 0.25, 1), (0.25, 0.25, 1), (0.75, 0.25, 1)], True, "two equal columns: det = 0 exactly, not > 0",
             model=True, mirror=True),
        Case("det_x_equals_y", "det", [(1, 1, 4), (2, 2, 8), (-1, -1, 4)], True, "the x row equals the y row, small integers: det = 0 exactly", model=True, mirror=True),
        Case("det_zero", "det", [(0, 0, 1), (1, 0, 1), (0.5, 0, 1)], True, "det = e with e = 0", model=True),
        Case("det_plus_smallest", "det", [(0, 0, 1), (1, 0, 1), (0.5, u, 1)], False, "det = (0 - 1 * (0 - e)) + 0.5 * 0 = e = +unit > 0"),
        Case("det_minus_smallest", "det", [(0, 0, 1), (1, 0, 1), (0.5, -u, 1)], True, "det = e = -unit"),
        Case("det_all_w_negative_front_order", "det", [(0.25, 0.25, -1), (0.25, 0.75, -1), (0.75, 0.25, -1)], False,
             "the surviving filler with every w negated: det changes sign with w0 w1 w2: +0.25", model=True, mirror=True),
        Case("det_all_w_negative_swapped", "det", [(0.25, 0.25, -1), (0.75, 0.25, -1), (0.25, 0.75, -1)], True, "and the culled filler survives: -0.25",
             model=True, mirror=True),
        # (t0 - t1) + t2 against t0 - (t1 - t2): all w = 1, so the cofactors are y1 - y2, y0 - y2, y0 - y1
        Case("det_association_positive_as_written", "det", [(0.5, 0.5, 1), (1, 1, 1), (-(2.0 ** -25), 0, 1)], False,
             "t = 0.5, 0.5, 2^-26: (t0 - t1) + t2 = 2^-26 > 0; t1 - t2 rounds (to even) to 0.5, so t0 - (t1 - t2) = 0", model=True, mirror=True),
        Case("det_association_zero_as_written", "det", [(2.0 ** -25, 1, 1), (0.5, 0.5, 1), (1, 0, 1)], True,
             "t = 2^-26, 0.5, 0.5: t0 - t1 rounds to -0.5, + t2 = 0; t0 - (t1 - t2) = 2^-26 > 0", model=True, mirror=True),
    ]
    # One cancelling cofactor each: y_i w_j - y_j w_i is 0 in float32 and +-2^-24 exact, the other two corners' x are 0 so det
    # is that cofactor times the third corner's x. A: the FIRST product is inexact (a * a), B: the second — a contraction keeps
    # one of the two products exact, which one is the compiler's choice. The sign of x makes the contracted det positive.
    for (i, j, k), sign in (((1, 2, 0), 1), ((0, 2, 1), -1), ((0, 1, 2), 1)):       # cofactor (i, j) is multiplied by sign * x_k
        for variant in "AB":
            c = [[F(0), F(0), F(1)] for _ in range(3)]
            if variant == "A":
                c[i][1], c[j][2], c[j][1], c[i][2] = a, a, b2, F(1)      # a * a - b2 * 1
                exact = 1
            else:
                c[i][1], c[j][2], c[j][1], c[i][2] = F(1), b2, a, a      # 1 * b2 - a * a
                exact = -1
            c[k][0] = F(sign * exact)
            out.append(Case(f"det_cancelling_cofactor_{i}{j}_{variant}", "det", c, True,
                            "the cofactor is 0 in float32 (a * a rounds to 1 + 2^-11): det = 0; with that subtraction contracted it is +-2^-24 "
                            "and det = +2^-24 > 0", model=True, mirror=True))
    return out


def _nan_cases():
    """Group "scaled" only. A NaN VERTEX would make the geometry non-finite, and a non-finite geometry sends every command of
    the context down the literal chain: the affine instantiation would never run. So a NaN corner comes from the finite vertex
    (2^127, 2^127, 1) by overflow under the scale-2 instance: world.x = world.y = +inf, and every row of pv then holds a
    -0 * inf = NaN: clip = (NaN, NaN, NaN). Only a model matrix that scales can do this; under the identity instance no entry of
    these pv matrices (+-0, +-1, +-4) makes a NaN from finite vertices."""
    n = (NAN, NAN, NAN)
    return [
        Case("nan_one_corner_of_a_back_face", "nan", [(0.25, 0.25, 1), n, (0.25, 0.75, 1)], True, "det is NaN: not > 0; no bound has all three", model=True),
        Case("nan_two_corners", "nan", [n, (0.75, 0.25, 1), n], True, "every comparison with NaN is false", model=True),
        Case("nan_three_corners", "nan", [n, n, n], True, "every comparison with NaN is false", model=True),
        Case("nan_corner_beside_two_beyond", "nan", [(3, 0.5, 1), n, (5, 0.25, 2)], True, "two corners beyond the right bound, the third is NaN: not all three",
             model=True),
    ]


def _infinite_cases():
    """Group "overflow" only: +-inf = 4 * +-2^127."""
    out = []
    for sg, name in ((1, "plus"), (-1, "minus")):
        i = F(sg) * INF
        out += [
            Case(f"inf_w_{name}_all", "inf", [(0.25, 0.25, i), (0.25, 0.75, i), (0.75, 0.25, i)], True,
                 "x / inf = 0: inside; every cofactor is inf - inf = NaN: det is NaN"),
            Case(f"inf_x_{name}_all_finite_w_positive", "inf", [(i, 0.25, 1), (i, 0.5, 1), (i, 1, 2)], False, "x / w = +-inf for all three"),
            Case(f"inf_x_{name}_all_finite_w_negative", "inf", [(i, 0.25, -1), (i, 0.5, -1), (i, 1, -2)], False, "x / w = -+inf for all three"),
            Case(f"inf_y_{name}_all", "inf", [(0.25, i, 1), (0.5, i, 1), (1, i, 2)], False, "y / w = +-inf for all three"),
            Case(f"inf_x_{name}_over_inf_w", "inf", [(i, 0.25, INF), (i, 0.5, INF), (i, 1, INF)], True,
                 "inf / inf = NaN: beyond no bound (the kernel's inf > inf is false too); det is NaN"),
            Case(f"inf_x_{name}_one_corner", "inf", [(i, 0.5, 1), (F(sg) * 3, 0.5, 1), (F(sg) * 5, 0.25, 2)], False,
                 "x / w = +-inf, +-3, +-2.5: all beyond the same bound, whatever the determinant"),
            Case(f"inf_y_{name}_one_corner", "inf", [(0.5, i, 1), (0.25, F(sg) * 5, 2), (0.5, F(sg) * 3, 1)], False,
                 "y / w = +-inf, +-2.5, +-3: all beyond the same bound, whatever the determinant"),
        ]
    out += [
        Case("inf_w_one_corner_det_plus_inf", "inf", [(0.5, -0.5, 1), (0.5, 0.5, 1), (0.25, 0.25, INF)], False,
             "t0 = 0.5 (0.5 inf - 0.25) = +inf, t1 = 0.5 (-0.5 inf - 0.25) = -inf: det = +inf > 0"),
        Case("inf_w_one_corner_det_minus_inf", "inf", [(0.5, 0.5, 1), (0.5, -0.5, 1), (0.25, 0.25, INF)], True, "det = -inf; x / w = 0.5, 0.5, 0"),
    ]
    return out


FRONT = [(0.25, 0.25, 1), (0.25, 0.75, 1), (0.75, 0.25, 1)]      # det = 0.25 (0.75 - 0.25) - 0 + 0.75 (0.25 - 0.75) = -0.25: kept
BACK = [FRONT[0], FRONT[2], FRONT[1]]                             # det = +0.25: culled
FILLER_FRONT = Case("filler_front", "filler", FRONT, True, "det = -0.25, NDC within 0.75")
FILLER_BACK = Case("filler_back", "filler", BACK, False, "det = +0.25")

_CASES = {}


def cases(group):
    """The catalogue of one group, in mesh order."""
    if group not in _CASES:
        g = GROUPS[group]
        if g["full"]:
            out = _ndc_cases(g) + _subnormal_cases(g) + _zero_w_cases(g) + _mixed_w_cases() + _det_cases(g)
            if group == "overflow":
                out += _infinite_cases()
        else:
            base = GROUPS["pos"]
            out = [c for c in _ndc_cases(base) + _mixed_w_cases() + _det_cases(base) + _nan_cases() if (c.mirror if group == "mirror" else c.model)]
            out += _zero_w_cases(g)
        assert len({c.name for c in out}) == len(out)
        _CASES[group] = out
    return _CASES[group]


def cases_of_pv(pv_name):
    return [(grp, c) for grp in GROUPS if PV_OF[grp] == pv_name for c in cases(grp)]


# The scenes the GPU tests run: (instances, the first instance's mesh) — one instance of either rotation, both, and 65 (two waves
# of commands and one more).
SCENES = [(1, 0), (1, 1), (2, 0), (65, 1)]


# ---- the builder ----------------------------------------------------------------------------------------------------------

def instance_arrays(group, n):
    i = GROUPS[group]["instance"]
    return (np.tile(np.array(i["pos"], F), (n, 1)), np.tile(np.array(i["rot"], F), (n, 1)), np.full(n, i["scale"], F))


def realise(group, corner):
    """The mesh vertex whose clip coordinates under the group's pv and instance are `corner` (x, y, w)."""
    g = GROUPS[group]
    x, y, w = (F(v) for v in corner)
    if np.isnan(x) or np.isnan(y) or np.isnan(w):                  # by overflow in the model matrix (_nan_cases): a FINITE vertex
        assert g["instance"] is SCALED_INSTANCE and np.isnan(x) and np.isnan(y) and np.isnan(w)
        return (F(2.0 ** 127), F(2.0 ** 127), F(1))
    pv = PVS[g["pv"]]
    px, py, pw = pv[0], pv[5], -pv[11]
    big = F(2.0 ** 127)

    def world(c, p):                                               # c = p * world; +-inf = p * +-2^127 (p = +-4)
        if np.isinf(c):
            assert abs(p) == 4
            return F(np.sign(c) * np.sign(p)) * big
        return F(F(c) / F(p)) + F(0)                               # (+ 0: a world zero is +0)
    wx, wy, wz = world(x, px), world(y, py), world(w, -pw)
    inst = g["instance"]
    if inst is tc.MIRROR_INSTANCE:                                 # world = (x, 2 - y, z)
        return (wx, F(F(2) - wy), wz)
    s, t = F(inst["scale"]), np.array(inst["pos"], F)
    return tuple(F(F(c - t[k]) / s) + F(0) for k, c in enumerate((wx, wy, wz)))


def layout(group, rotate=0):
    """The triangles of the group's mesh in order, as Case objects: the catalogue in two runs — the first from triangle 0 (so
    a case sits on lane 0 and another on lane 63 of the first step), the second across triangle 256 (a range cut under
    MIP_TUNE_TRI_RANGE_SLOTS=256) — padded with surviving and culled fillers in turn to a multiple of 64 triangles and at least
    four steps; then rolled by `rotate` (63: triangle k goes to k + 63 — one lane back, and all but a step's first into the next step)."""
    cs = cases(group)
    second = min(24, len(cs) // 3)
    first = cs[: len(cs) - second]
    fill = [FILLER_FRONT, FILLER_BACK]
    out = list(first)
    if len(out) < 64:                                              # a short catalogue: its last case of the run goes to lane 63
        out = out[:-1] + [fill[k % 2] for k in range(len(out) - 1, 63)] + out[-1:]
    for k in range(len(out), max(244, len(out) + 2)):
        out.append(fill[k % 2])
    out += cs[len(cs) - second:]
    while len(out) % 64 or len(out) < 256:
        out.append(fill[len(out) % 2])
    assert len(out) >= 256 + 12
    return list(np.roll(np.array(out, object), rotate))


def mesh(group, rotate=0):
    """(vertices (3 T, 3) float32, indices 0 .. 3 T - 1, the layout): three vertices of its own per triangle."""
    tris = layout(group, rotate)
    v = np.array([realise(group, c.clip[k]) for c in tris for k in range(3)], F).reshape(-1, 3)
    return v, np.arange(len(v), dtype=U32), tris


def scene(ra, group, n, rotations=(0, 63), nan_vertex=False, first_mesh=0):
    """n instances of the group's meshes (one mesh per rotation, dealt in turn from first_mesh on), under planes nothing fails, with the mesh
    table's own boxes. Returns dict(s — the scene, vertices, indices, pv, layouts — per mesh). nan_vertex: one NaN vertex that
    no index names is appended (the geometry is then not finite, and every command takes the literal chain)."""
    meshes = np.zeros(len(rotations), ra.MESH_DTYPE)
    vs, ixs, layouts = [], [], []
    v_off = i_off = 0
    for k, r in enumerate(rotations):
        v, ix, tris = mesh(group, r)
        meshes["aabb_min"][k], meshes["aabb_max"][k] = (-1, -1, -1), (1, 1, 1)
        meshes["n_lods"][k], meshes["index_len"][k, 0], meshes["index_offset"][k, 0], meshes["vertex_offset"][k] = 1, len(ix), i_off, v_off
        vs.append(v), ixs.append(ix), layouts.append(tris)
        v_off, i_off = v_off + len(v), i_off + len(ix)
    if nan_vertex:
        vs.append(np.full((1, 3), np.nan, F))
    pos, rot, scale = instance_arrays(group, n)
    planes = np.tile(np.array([0, 0, 0, -1], F), 6)                # sd - e = -1 for every box: nothing is outside
    s = dict(n=n, pos=pos, rot=rot, scale=scale, mesh_id=((np.arange(n) + first_mesh) % len(rotations)).astype(U32), meshes=meshes, planes=planes,
             cam_pos=np.zeros(3, F), base=0, bitmap=np.full((n + 31) // 32, 0xFFFFFFFF, U32))
    return dict(s=s, vertices=np.concatenate(vs), indices=np.concatenate(ixs), pv=PVS[PV_OF[group]], layouts=layouts, group=group)


def expected_stream(sc, capacity=None):
    """From the hand flags alone: (index count per instance, the culled index buffer of `capacity` words — instance i's surviving
    triangles in mesh order from word 3 T i on, the sentinel elsewhere; capacity None: only the surviving indices, in order)."""
    s = sc["s"]
    counts, chunks = [], []
    t3 = 3 * len(sc["layouts"][0])
    buf = None if capacity is None else np.full(capacity, SENTINEL, U32)
    for i in range(s["n"]):
        tris = sc["layouts"][int(s["mesh_id"][i])]
        kept = np.array([c.kept for c in tris], bool)
        ix = np.arange(3 * len(tris), dtype=U32).reshape(-1, 3)[kept].reshape(-1)
        counts.append(len(ix))
        chunks.append(ix)
        if buf is not None:
            buf[t3 * i : t3 * i + len(ix)] = ix
    return np.array(counts, np.int64), (np.concatenate(chunks) if buf is None else buf)


# ---- the float32 restatement with switches: every mutant is ONE mistake ------------------------------------------------------

def clip_of(model, pv, v):
    """clip (t, 3 corners, 4) of the triangles v (t, 3, 3) under the float32 chain of numpy_restatement.triangle_culled."""
    import numpy_restatement as nr

    m = [F(x) for x in np.asarray(model, F).reshape(16)]
    p = [F(x) for x in np.asarray(pv, F).reshape(16)]
    with np.errstate(all="ignore"):
        out = []
        for k in range(3):
            world = nr._mat4_vec4(m, v[:, k, 0], v[:, k, 1], v[:, k, 2], F(1.0))
            out.append(np.stack(nr._mat4_vec4(p, world[0], world[1], world[2], world[3]), axis=1))
    return np.stack(out, axis=1)


def kernel_ndc_outside(clip):
    """The kernel's division-free predicate (triangle_cull_clip): x and y take w's SIGN BIT, then compare with +-|w|."""
    sw = bits(clip[..., 3]) & U32(0x80000000)
    w = np.abs(clip[..., 3])
    with np.errstate(all="ignore"):
        x = (bits(clip[..., 0]) ^ sw).view(F)
        y = (bits(clip[..., 1]) ^ sw).view(F)
        return (x < -w).all(axis=1) | (x > w).all(axis=1) | (y < -w).all(axis=1) | (y > w).all(axis=1)


def culled(clip, mistake=None):
    """generate_work.comp:137-166 from the clip coordinates (t, 3, 4), in float32; `mistake` names one departure."""
    one = F(1.0)
    with np.errstate(all="ignore"):
        c = clip.astype(F)
        if mistake == "flush_subnormals":
            c = np.where((np.abs(c) < NORMAL_MIN) & ~np.isnan(c), np.copysign(F(0), c), c).astype(F)
        x, y, z, w = (c[..., k] for k in range(4))
        third = z if mistake == "det_xyz" else w

        def cofactor(i, j, which):
            if mistake == f"det_contracted_{which}":               # both products exact, one rounding
                return (y[:, i].astype(np.float64) * third[:, j].astype(np.float64) - y[:, j].astype(np.float64) * third[:, i].astype(np.float64)).astype(F)
            return y[:, i] * third[:, j] - y[:, j] * third[:, i]
        t0, t1, t2 = x[:, 0] * cofactor(1, 2, 0), x[:, 1] * cofactor(0, 2, 1), x[:, 2] * cofactor(0, 1, 2)
        det = t0 - (t1 - t2) if mistake == "det_reassociated" else (t0 - t1) + t2
        cull = det >= F(0) if mistake == "det_ge" else det > F(0)
        if mistake == "ndc_reciprocal":
            r = one / w
            qx, qy = x * r, y * r
        elif mistake == "no_sign_flip":
            qx, qy = x / np.abs(w), y / np.abs(w)
        elif mistake == "sign_by_compare":                         # the kernel's predicate with `w < 0` for the sign bit
            neg = w < F(0)
            wa = np.abs(w)
            qx, qy, one = np.where(neg, -x, x), np.where(neg, -y, y), wa
        else:
            qx, qy = x / w, y / w
        if mistake == "ndc_ge":
            lo_x, hi_x, lo_y, hi_y = qx <= -one, qx >= one, qy <= -one, qy >= one
        else:
            lo_x, hi_x, lo_y, hi_y = qx < -one, qx > one, qy < -one, qy > one
        if mistake == "any_corner_outside":
            outside = lo_x.any(axis=1) | hi_x.any(axis=1) | lo_y.any(axis=1) | hi_y.any(axis=1)
        elif mistake == "sides_mixed":
            outside = (lo_x | hi_x | lo_y | hi_y).all(axis=1)
        elif mistake == "y_bound_missing":
            outside = lo_x.all(axis=1) | hi_x.all(axis=1)
        else:
            outside = lo_x.all(axis=1) | hi_x.all(axis=1) | lo_y.all(axis=1) | hi_y.all(axis=1)
        out = cull | outside
        if mistake == "nan_culled":                                # a comparison with NaN taken as true: a NaN det, a NaN quotient
            out = out | np.isnan(det) | np.isnan(qx).any(axis=1) | np.isnan(qy).any(axis=1)
    return out


MUTANTS = ["det_ge", "det_contracted_0", "det_contracted_1", "det_contracted_2", "det_reassociated", "det_xyz", "ndc_ge", "ndc_reciprocal",
           "no_sign_flip", "sign_by_compare", "flush_subnormals", "any_corner_outside", "sides_mixed", "y_bound_missing", "nan_culled"]
mutants = {name: (lambda clip, name=name: culled(clip, name)) for name in MUTANTS}
