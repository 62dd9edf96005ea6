"""The figures of profiles/entry_bounds.txt, measured on the GPU without asserting anything: for every case of the
point-wise layers' GPU tests -- the frame transforms, the point projection, the depth lift, the hard projection, the plane
fit, and the camera gradients of their edge cases -- the worst ratio of an error to its per-entry bound
(tests/entry_checks.py), and the plane fit's C64: the largest (|got - ref| - 2^-24 |ref|) / max|ref| against the fp64
oracle over every entry of every normals case.

    python tools/measure_entry_bounds.py [--out DIR]      # DIR gets entry_bounds_measure.txt and .json"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import entry_checks as ec
import frames_cases as fc, surfels_cases as sc, hard_projection_cases as hc, normals_cases as nc, normals_edge_cases as ne
import surfels_edge_cases as se, hard_projection_edge_cases as he, hard_projection_oracle as ho, surfels_oracle as so
import camera_edge_cases as ce
import test_hip_frames as fr, test_hip_surfels as ts, test_hip_hard_projection as th, test_hip_normals as tn
import test_hip_camera_edges as tce

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
worst = {}
lines = []

def note(layer, what, tag, got, ref, A, floor=ec.C):
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    A = np.broadcast_to(np.asarray(A, np.float64), ref.shape)
    ok = np.isfinite(ref)
    pattern = bool(np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~ok & ~np.isnan(ref)], ref[~ok & ~np.isnan(ref)]))
    with np.errstate(invalid="ignore", over="ignore"):
        r = ec.ratios(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), np.where(ok, A, 0.0), floor)[ok]
    w = float(r.max(initial=0.0))
    key = f"{layer}, {what}"
    worst[key] = max(worst.get(key, 0.0), w)
    lines.append(f"{key:34s} {tag:48s} dtype {got.dtype} worst {w:.4g} beyond {int((r > 1).sum())}/{r.size} pattern_ok {pattern}")
    print(lines[-1], flush=True)

# frames
for name in fc.TRANSFORM:
    for d in fc.DIRECTIONS:
        got = fr.transform(fc.transform_case(name), d, camera_grad=True)
        want, A = fc.transform_expected(name, d), fc.transform_magnitudes(name, d)
        for what, g, w, a in zip(("values", "gradients", "camera"), got, want, A):
            for k in w:
                note("frames transform", what, f"{name} {d} {k}", g[k], w[k], a[k])
for name in fc.PROJECT:
    for coords in (False, True):
        got = fr.project(fc.project_case(name), coords, camera_grad=True)
        want, A = fc.project_expected(name, coords), fc.project_magnitudes(name, coords)
        for what, g, w, a in zip(("values", "gradients", "camera"), got, want, A):
            for k in a:
                note("frames project", what, f"{name} {coords} {k}", g[k], w[k], a[k])
# surfels
import test_hip_camera_warp as cw
for name, variant in sc.ALL:
    c = sc.case(name, variant)
    got, got_g = ts._hip(c)
    (want, want_g), (A, A_g, A_c) = sc.expected(name, variant), sc.magnitudes(name, variant)
    note("surfels", "values", sc.tag(name, variant), got["pos"], want["pos"], A["pos"])
    note("surfels", "gradients", sc.tag(name, variant), got_g["depth"], want_g["depth"], A_g["depth"])
    if c["frame"] == "world":
        _, _, cam = cw.lift(c)
        want_c = ce.co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"], "world")[2]["camera"]
        for k in want_c:
            note("surfels", "camera", f"{sc.tag(name, variant)} {k}", ec.narrowed(cam["camera"][k]), want_c[k], A_c[k])
for name in se.NAMES:
    c = se.case(name)
    got, got_g = ts._hip(c)
    want, want_g = se.expected(name)
    A, A_g, _ = so.magnitudes({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"])
    note("surfels edges", "values", name, got["pos"], want["pos"], A["pos"])
    note("surfels edges", "gradients", name, got_g["depth"], want_g["depth"], A_g["depth"])
# hard projection
for mod, names in ((hc, hc.NAMES), (he, he.NAMES)):
    for name in names:
        c = mod.case(name)
        got, got_g = th._hip(c)
        want, want_g = mod.expected(name)
        A, A_g = ho.magnitudes({"surfels": c["surfels"], "rgb": c["rgb"]}, c["camera"], c["upstream"])
        note("hard projection", "values", name, got["out"], want["out"], A["out"])
        note("hard projection", "gradients", name, got_g["rgb"], want_g["rgb"], A_g["rgb"])
# normals: C64
c64 = 0.0
for mod, items in ((nc, nc.ALL), (ne, [(n,) for n in ne.NAMES])):
    for item in items:
        c = mod.case(*item)
        got, got_g = tn._hip(c)
        want, want_g = mod.expected(*item)
        again, again_g = mod.turned(*item)
        tag = " ".join(str(i) for i in item)
        for what, g, w, a2 in (("values", got["normal"], want["normal"], again["normal"]), ("gradients", got_g["pos"], want_g["pos"], again_g["pos"])):
            fin = np.isfinite(w)
            scale = float(np.abs(w[fin]).max()) if fin.any() else 0.0
            with np.errstate(invalid="ignore"):
                ill = fin & ec.ill_conditioned(w, a2, scale)
            held = fin & ~ill
            excess = (np.abs(g.astype(np.float64) - w) - 2.0 ** -24 * np.abs(w))[held]
            m = float(excess.max(initial=0.0)) / scale if scale > 0 else float(np.abs(g[held]).max(initial=0.0))
            c64 = max(c64, m)
            lines.append(f"normals {what:10s} {tag:30s} scale {scale:.4g} max excess/scale {m:.4g} = 2^{np.log2(m) if m > 0 else -np.inf:.2f} ill {int(ill.sum())}")
            print(lines[-1], flush=True)
            note("normals", what, tag, g, w, scale, ec.NORMALS_C64)
lines.append(f"normals measured max excess / scale = {c64:.6g} = 2^{np.log2(c64):.3f}; x4 = {4 * c64:.6g} = 2^{np.log2(4 * c64):.3f}; cap 2^-36 = {2.0 ** -36:.6g}")
print(lines[-1], flush=True)
# camera edge rows
for layer, name, variant in ce.ALL:
    sub = ce._layer_of(layer, name)
    if sub not in tce.PER_ENTRY:
        continue
    got = tce.full(layer, name, variant)
    want, A = ce.expected(layer, name, variant), ce.magnitudes(layer, name, variant)
    rows = [0, 2] if layer == "poisoned" else slice(None)
    for k in ce.KEYS:
        if np.isfinite(want[2][k][rows]).all():
            note(f"camera edges {sub}", "camera", f"{ce.tag(layer, name, variant)} {k}", ec.narrowed(got[2][k])[rows], want[2][k][rows], A[2][k][rows])
lines.append("")
lines += [f"WORST {k}: {v:.4g}" for k, v in sorted(worst.items())]
if OUT is not None:
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "entry_bounds_measure.txt"), "w").write("\n".join(lines) + "\n")
    json.dump({"worst": worst, "normals_c64_measured": c64}, open(os.path.join(OUT, "entry_bounds_measure.json"), "w"), indent=1)
print("\n".join(lines[-20:]))
