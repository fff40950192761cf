"""Known answers of the per-triangle test (generate_work.comp:137-166), small enough to verify on paper.

The default camera sits at (0, 1, 2) and looks down +z with the identity rotation, so with the identity model matrix
the clip coordinates of a world point (x, y, z) are

    clip.x = a * x,   clip.y = b * (y - 1),   clip.w = z - 2        a = 1 / (2 tan 35 deg) = 0.71407...,  b = 2 a

(scene.default_pv(); clip.z is never tested). NDC = clip.xy / clip.w, and the x / y bounds are |NDC| = 1: at w = 10
(z = 12) that is |x| = 14.004 and |y - 1| = 7.002.

Which winding survives. The shader culls when det(mat3(v0.xyw, v1.xyw, v2.xyw)) > 0 and calls that "backface culling in
counter clockwise front-facing order" (:142-143). That determinant is w0 w1 w2 times the doubled signed area of the
triangle in the (NDC.x, NDC.y) plane drawn with y UP: positive for corners that run counter-clockwise in that drawing,
when all w are positive. Vulkan's framebuffer has y DOWN, which mirrors the drawing: counter-clockwise with y up is
clockwise on the screen. So a triangle in front of the camera whose corners run counter-clockwise ON SCREEN has det < 0
and is kept, and the same triangle with two corners swapped is culled — which is what the shader's comment says.

`tri(cx, cy, z, h)` is (cx - h, cy, z), (cx, cy + 2h, z), (cx + h, cy, z): left, top, right in world space = left, BOTTOM,
right on screen (larger y is further down): counter-clockwise on screen, the front-facing order.
"""
import numpy as np


def tri(cx, cy, z, h=1.0):
    return [(cx - h, cy, z), (cx, cy + 2 * h, z), (cx + h, cy, z)]


def swapped(t):
    return [t[0], t[2], t[1]]


NAN = float("nan")

# (name, corners, kept by the shader under the identity model and default_pv(), why)
CASES = [
    ("front_ccw_on_screen", tri(0, 1, 12), True, "det < 0, NDC within +-0.15"),
    ("front_two_corners_swapped", swapped(tri(0, 1, 12)), False, "det > 0"),
    ("left_of_frustum", tri(-30, 1, 12), False, "NDC.x = a * (-31 .. -29) / 10 < -1 for all three"),
    ("right_of_frustum", tri(30, 1, 12), False, "NDC.x > 1 for all three"),
    ("above_frustum", tri(0, 20, 12), False, "NDC.y = b * (19 .. 21) / 10 > 1 for all three"),
    ("below_frustum", tri(0, -20, 12), False, "NDC.y < -1 for all three"),
    ("straddles_x_bound", tri(14.5, 1, 12), True, "NDC.x = 0.964, 1.035, 1.107: not all beyond the bound"),
    ("straddles_y_bound", tri(0, 7, 12), True, "NDC.y = 0.857, 1.142, 0.857"),
    ("beyond_far_plane", tri(0, 1, 200), True, "w = 198 > far = 100: z is not tested"),
    ("in_front_of_near_plane", tri(0, 0.99, 2.05, h=0.01), True, "w = 0.05 < near = 0.1, |NDC| < 0.3: z is not tested"),
    # all w = -10: det = w0 w1 w2 x (doubled NDC area) changes sign with the product of the w; NDC = clip / -10 lies inside
    ("behind_camera_front_order", tri(0, 1, -8), False, "w < 0 for all three flips the determinant's sign: det > 0"),
    ("behind_camera_swapped", swapped(tri(0, 1, -8)), True, "det < 0, NDC = clip / -10 inside the bounds"),
    ("behind_camera_left_swapped", swapped(tri(-30, 1, -8)), False, "det < 0, but x / w = a * (-31 .. -29) / -10 > 1: the division flips the side"),
    # corner 1 has w = 0 exactly (z = 2): x / 0 = +inf, y / 0 = +inf
    ("one_corner_w_zero_inside", [(-1, 1, 12), (0.5, 3, 2), (1, 1, 12)], True,
     "det = -a * 10 * 2b - a * 10 * 2b < 0; NDC.x = -0.07, +inf, 0.07: no bound has all three beyond it"),
    ("one_corner_w_zero_right", [(20, 1, 12), (25, 1, 2), (22, 1, 12)], False, "NDC.x = 1.43, +inf, 1.57: all > 1 (and y = 0 everywhere: det = 0)"),
    ("nan_corner", [(-1, 1, 12), (NAN, 3, 12), (1, 1, 12)], True, "every comparison with NaN is false"),
    ("zero_area", [(-1, 1, 12), (-1, 1, 12), (1, 1, 12)], True, "two equal columns: det = 0 exactly, not > 0; the degenerate test is disabled (:166)"),
]

# A mirrored instance: scale -1 and a half turn about y give M = diag(1, -1, 1) (+ translation (0, 2, 0)): y -> 2 - y. The
# triangle keeps its place on screen upside down, its winding reverses, and the decision flips.
MIRROR_INSTANCE = dict(pos=(0.0, 2.0, 0.0), rot=(0.0, 1.0, 0.0, 0.0), scale=-1.0)
MIRROR_CASES = [
    ("mirrored_front_order", tri(0, 1, 12), False, "y -> 2 - y reverses the winding: det > 0"),
    ("mirrored_swapped", swapped(tri(0, 1, 12)), True, "and the swapped triangle is now front-facing"),
]


def case_mesh(cases=CASES):
    """The cases as one tiny mesh: three vertices per triangle, indices 0 .. 3 T - 1."""
    vertices = np.array([c for _, corners, _, _ in cases for c in corners], np.float32).reshape(-1, 3)
    return vertices, np.arange(len(vertices), dtype=np.uint32)
