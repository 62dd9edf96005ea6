"""Edge inputs for the regulariser tests, generated, not stored: the shapes, conventions, non-finite inputs and one-hot
upstream weights that tests/regularizer_cases.py does not reach.  Used by tests/test_regularizer_edge_cases_cpu.py (which
pins what the fp64 restatement says of each), tests/test_regularizers_host_cpu.py (the host build of the per-pixel
arithmetic) and tests/test_hip_regularizers_edges.py (the GPU).

A case is the dict of regularizer_cases.py: the four fp32-representable inputs with the view axis, z_min / z_max /
z_scale / unit_normal_scale, weights (B, 7), `flat` (H, W) bool or None marking the pixels whose exact zeros are the
convention under test, `single` False.  Two more keys: `designed`, the (row, column) pixels a convention case was
built around (`marks` names subsets of them), and `poison`, (input, view, row, column, component or None, clean value) of a poisoned case.

Shape cases: random values, the smallest shapes that reach the branch (nblk = workgroups of 256 pixels per view)
    2x300, 300x2     multiplicity 2 on one axis only; rows that change every second lane / two rows over two workgroups
    2x8257_b2        65 workgroups, two rows, two views
    129x128          65 workgroups: k_reg_finish's lane 0 adds rows 0 and 64, lane 1 only row 1
    130x127_b3       65 workgroups, ragged last one, three views with distinct weights
Convention cases: one designed pixel or block (`designed`, `flat`) in an otherwise random 6 x 7 view
    coincident_3x3   nine equal positions: d_k = 0, u_k = 0 and sign(0) in the forty pairs inside the block
    origin           p = 0: n . p = 0 and |p_z| = 0
    pz_zero          p_z = 0 alone
    n_dot_p_zero     p = (0, 1, -3), n = (1, 0, 0)
    zmin_eq_zmax     z_min = z_max = 3 and one p_z = -3
    const_pos        every position (0.25, -0.5, -3): variance 0, spatial_var = 1e4
    huge_pos         one pixel at (1e18, -1e18, -1e19)
    tiny_pos         positions x 1e-20, z_min = 0
    corner_conventions_2x5, corner_conventions_5x2
                     image 0 / constant depth over the two corners of one short edge and their neighbours, |p_z| = z_min
                     and = z_max at the other two corners, |p_z| = z_min on a long edge: every neighbour is a reflection
Poisoned cases: three 6 x 7 views, the middle one with one non-finite entry, the outer ones random
    nan_pos, inf_normal, inf_depth, nan_image   at the interior pixel (2, 3)
    nan_pos_corner                              at (0, 0), which is p_0 of the variance
One-hot weights: onehot_<term> = the inputs of regularizer_cases' 17x9_b3 with that term's weights alone.

Kink condition: as regularizer_cases.py, MARGIN = 1e-9 clear of every kink outside `flat`, redrawn from the next seed if
not.  Two cases measure it on a twin: a poisoned view on its clean values (a NaN has no margin; every quantity that
does not read the poisoned entry is the twin's), and tiny_pos on its positions times 1e20 in fp64 (every decision
quantity is homogeneous in pos once z_min = 0, so this is the relative clearance of the actual inputs; the absolute one
is 1e-29).

PINS states, per poisoned case, what the restatement gives for the poisoned view: the class of each term ("finite",
"+inf", "-inf", "nan") and where each gradient array is finite ("all", "none", "outside_block" = outside the poisoned
pixel's 3 x 3 block clipped to the view, "outside_pixel").  tests/test_regularizer_edge_cases_cpu.py asserts that the
restatement does give exactly that; the host and GPU tests compare where finite_mask() says, never where the code under
test happens to be finite."""
import functools

import numpy as np

import regularizer_cases as cases
import regularizer_oracle as ro

MARGIN = cases.MARGIN
SHAPE_NAMES = ("2x300", "300x2", "2x8257_b2", "129x128", "130x127_b3")
CONVENTION_NAMES = ("coincident_3x3", "origin", "pz_zero", "n_dot_p_zero", "zmin_eq_zmax", "const_pos", "huge_pos",
                    "tiny_pos", "corner_conventions_2x5", "corner_conventions_5x2")
POISONED_NAMES = ("nan_pos", "inf_normal", "inf_depth", "nan_image", "nan_pos_corner")
ONEHOT_NAMES = tuple("onehot_" + t for t in ro.TERMS)
NAMES = SHAPE_NAMES + CONVENTION_NAMES + POISONED_NAMES + ONEHOT_NAMES
_SHAPES = {"2x300": (1, 2, 300), "300x2": (1, 300, 2), "2x8257_b2": (2, 2, 8257), "129x128": (1, 129, 128),
           "130x127_b3": (3, 130, 127), "corner_conventions_2x5": (1, 2, 5), "corner_conventions_5x2": (1, 5, 2)}
PIXEL = (2, 3)                        # the designed / poisoned interior pixel of a 6 x 7 view
CONST_POINT = (0.25, -0.5, -3.0)
HUGE_POINT = (1e18, -1e18, -1e19)
TINY = 1e-20

_NAN5 = {"z": "nan", "unit_normal": "finite", "normal_consistency": "nan", "spatial": "nan", "spatial_var": "nan",
         "image_depth_consistency": "finite", "away_from_camera": "nan"}
_FINITE = {t: "finite" for t in ro.TERMS}
_ALL = {k: "all" for k in ro.INPUTS}
PINS = {
    "nan_pos": {"terms": _NAN5, "grads": dict(_ALL, pos="none", normal="outside_block")},
    "nan_pos_corner": {"terms": _NAN5, "grads": dict(_ALL, pos="none", normal="outside_block")},
    "inf_normal": {"terms": dict(_FINITE, unit_normal="+inf", normal_consistency="+inf", away_from_camera="+inf"),
                   "grads": dict(_ALL, pos="outside_block", normal="outside_pixel")},
    "inf_depth": {"terms": dict(_FINITE, image_depth_consistency="+inf"), "grads": _ALL},
    "nan_image": {"terms": dict(_FINITE, image_depth_consistency="nan"), "grads": _ALL},
}


# Exact zeros of the conventions: (case, the one term whose upstream weight is kept -- None: the case's own weights --,
# gradient arrays, which of the case's `marks`).  Every listed array is exactly 0.0 at every marked pixel.
EXACT_ZEROS = (
    ("zmin_eq_zmax", "z", ("pos",), "designed"),                      # relu'(0) = 0 on both sides
    ("pz_zero", "z", ("pos",), "designed"),                           # |.|'(0) = 0
    ("origin", "z", ("pos",), "designed"),
    ("n_dot_p_zero", "away_from_camera", ("pos", "normal"), "designed"),
    ("origin", "away_from_camera", ("pos", "normal"), "designed"),
    ("coincident_3x3", "normal_consistency", ("pos", "normal"), "centre"),      # all eight d_k = 0
    ("coincident_3x3", "spatial", ("pos",), "centre"),
    ("const_pos", "normal_consistency", ("pos", "normal"), "designed"),
    ("const_pos", "spatial", ("pos",), "designed"),
    ("const_pos", "spatial_var", ("pos",), "designed"),               # p - mean p = 0
    ("corner_conventions_2x5", "z", ("pos",), "z"),
    ("corner_conventions_5x2", "z", ("pos",), "z"),
    ("corner_conventions_2x5", None, ("image", "depth"), "still_corners"),      # every neighbour is still as well
    ("corner_conventions_5x2", None, ("image", "depth"), "still_corners"),
)


# the inputs each term depends on: under one-hot upstream weights the other gradients are exactly 0
REACH = {"z": {"pos"}, "unit_normal": {"normal"}, "normal_consistency": {"pos", "normal"}, "spatial": {"pos"},
         "spatial_var": {"pos"}, "image_depth_consistency": {"image", "depth"}, "away_from_camera": {"pos", "normal"}}


def one_hot(c, term):
    """The case with the upstream weights of every other term set to 0 (term None: the case itself)."""
    if term is None:
        return c
    w = np.zeros_like(c["weights"])
    k = ro.TERMS.index(term)
    w[:, k] = c["weights"][:, k]
    return dict(c, weights=w)


def nblk(c):
    """Workgroups of 256 pixels per view."""
    _, H, W = c["depth"].shape
    return (H * W + 255) // 256


def classify(v):
    """'finite', '+inf', '-inf' or 'nan' per element."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), "nan", np.where(np.isfinite(v), "finite", np.where(v > 0, "+inf", "-inf")))


def _base(shape, rng):
    """The random view of regularizer_cases: positions in front of the camera, weights of either sign."""
    B, H, W = shape
    pos = np.stack([rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape), -rng.uniform(1.5, 4.5, shape)], -1)
    c = {"pos": pos, "normal": rng.uniform(-1, 1, (B, H, W, 3)), "image": rng.uniform(0, 1, (B, H, W, 3)),
         "depth": rng.uniform(1, 5, shape), "z_min": 2.0, "z_max": 4.0, "z_scale": 2.0, "unit_normal_scale": 10.0,
         "flat": None, "single": False, "designed": (), "poison": None}
    c["weights"] = rng.uniform(0.5, 2.0, (B, 7)) * rng.choice([-1.0, 1.0], (B, 7))
    return c


def _mask(shape, pixels):
    m = np.zeros(shape, dtype=bool)
    for p in pixels:
        m[p] = True
    return m


def _corner_conventions(c, transposed):
    """On a 2 x 5 view (a 5 x 2 one if `transposed`), (short, long) coordinates."""
    at = (lambda s, l: (l, s)) if transposed else (lambda s, l: (s, l))
    still = [at(0, 0), at(1, 0), at(0, 1), at(1, 1)]                   # two corners and their neighbours
    for p in still:
        c["image"][(0,) + p] = 0.0
        c["depth"][(0,) + p] = 2.25
    c["pos"][(0,) + at(0, 4) + (2,)] = -c["z_min"]
    c["pos"][(0,) + at(1, 4) + (2,)] = -c["z_max"]
    c["pos"][(0,) + at(0, 2) + (2,)] = -c["z_min"]                       # on the long edge
    c["designed"] = tuple(still + [at(0, 4), at(1, 4), at(0, 2)])
    c["marks"] = {"still_corners": (at(0, 0), at(1, 0)), "z": (at(0, 4), at(1, 4), at(0, 2))}


def _draw(name, seed):
    rng = np.random.RandomState(seed)
    if name in ONEHOT_NAMES:
        return one_hot(dict(cases.case("17x9_b3"), designed=(), marks={}, poison=None), ro.TERMS[ONEHOT_NAMES.index(name)])
    c = _base(_SHAPES.get(name, (3, 6, 7) if name in POISONED_NAMES else (1, 6, 7)), rng)
    i, j = PIXEL
    if name == "coincident_3x3":
        c["pos"][0, i - 1:i + 2, j - 1:j + 2] = c["pos"][0, i, j]
        c["designed"] = tuple((a, b) for a in range(i - 1, i + 2) for b in range(j - 1, j + 2))
    elif name == "origin":
        c["pos"][0, i, j] = 0.0
    elif name == "pz_zero":
        c["pos"][0, i, j, 2] = 0.0
    elif name == "n_dot_p_zero":
        c["pos"][0, i, j] = (0.0, 1.0, -3.0)
        c["normal"][0, i, j] = (1.0, 0.0, 0.0)
    elif name == "zmin_eq_zmax":
        c.update(z_min=3.0, z_max=3.0)
        c["pos"][0, i, j, 2] = -3.0
    elif name == "const_pos":
        c["pos"][0] = CONST_POINT
        c["designed"] = tuple((a, b) for a in range(6) for b in range(7))
    elif name == "huge_pos":
        c["pos"][0, i, j] = HUGE_POINT
    elif name == "tiny_pos":
        c["pos"] = cases._f32(c["pos"]).astype(np.float64) * TINY
        c["z_min"] = 0.0
        c["margin_pos_scale"] = 1.0 / TINY
    elif name.startswith("corner_conventions"):
        _corner_conventions(c, name.endswith("5x2"))
    if name in CONVENTION_NAMES and name not in ("huge_pos", "tiny_pos") and not c["designed"]:
        c["designed"] = (PIXEL,)
    c["marks"] = dict(c.get("marks", {}), designed=c["designed"], centre=(PIXEL,))
    if c["designed"]:
        c["flat"] = _mask(c["depth"].shape[1:], c["designed"])
    for k in ro.INPUTS + ("weights",):
        c[k] = cases._f32(c[k])
    if name in POISONED_NAMES:
        key = {"nan_pos": "pos", "nan_pos_corner": "pos", "inf_normal": "normal", "inf_depth": "depth",
               "nan_image": "image"}[name]
        pi, pj = (0, 0) if name == "nan_pos_corner" else PIXEL
        comp = {"nan_pos": 2, "nan_pos_corner": 2, "inf_normal": 0, "nan_image": 1, "inf_depth": None}[name]
        at = (1, pi, pj) if comp is None else (1, pi, pj, comp)
        bad = np.float32(np.nan if name.startswith("nan") else np.inf)
        if name == "inf_normal":
            bad = np.copysign(bad, c["pos"][1, pi, pj, 0])           # n . p = +inf: the penalty fires
        c["poison"] = (key, 1, pi, pj, comp, c[key][at].copy())
        c[key][at] = bad
    return c


def clean(c):
    """The case with its poison taken out again (the case itself when it has none)."""
    if c["poison"] is None:
        return c
    key, b, i, j, comp, value = c["poison"]
    twin = dict(c, **{key: c[key].copy()}, poison=None)
    twin[key][(b, i, j) if comp is None else (b, i, j, comp)] = value
    return twin


def margins(c):
    """decision_margin of every view, on the twin described in the module docstring where the case has one."""
    twin = clean(c)
    if "margin_pos_scale" in c:
        twin = dict(twin, pos=twin["pos"].astype(np.float64) * c["margin_pos_scale"])
    return cases.margins(twin)


@functools.lru_cache(maxsize=None)
def case(name):
    first = 100000 + 1000 * NAMES.index(name)
    for seed in range(first, first + 50):
        c = _draw(name, seed)
        m = margins(c)
        if min(m) >= MARGIN:
            c.update(seed=seed, margins=m)                           # per view, as measured: the large cases take seconds
            return c
    raise RuntimeError(f"no draw of {name} keeps {MARGIN} clear of every kink")


def view(c, b):
    """View b of a case as a case of its own."""
    return dict(c, **{k: c[k][b:b + 1] for k in ro.INPUTS}, weights=c["weights"][b:b + 1], poison=None)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {term: (B,)}, gradients {input: (B, ...)}) of a case from the fp64 oracle, computed once."""
    c = case(name)
    return ro.gradients({k: c[k] for k in ro.INPUTS}, c["weights"], c["z_min"], c["z_max"], c["z_scale"],
                        c["unit_normal_scale"])


def block(c, i, j):
    """(H, W) bool: the 3 x 3 block around (i, j), clipped to the view."""
    _, H, W = c["depth"].shape
    m = np.zeros((H, W), dtype=bool)
    m[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True
    return m


def finite_mask(name, key):
    """Where PINS says the restatement's gradient `key` of case `name` is finite: a bool array of the gradient's
    shape.  All True for a case without poison."""
    c = case(name)
    m = np.ones(c[key].shape, dtype=bool)
    if c["poison"] is None:
        return m
    _, b, i, j, _, _ = c["poison"]
    how = PINS[name]["grads"][key]
    if how == "none":
        m[b] = False
    elif how == "outside_block":
        m[b][block(c, i, j)] = False
    elif how == "outside_pixel":
        m[b, i, j] = False
    else:
        assert how == "all", how
    return m
