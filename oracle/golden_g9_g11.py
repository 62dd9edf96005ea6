"""Generate tests/golden/g9_torch_autograd.npz, g10_torch_autograd_phong*.npz and g11_torch_autograd_ortho.npz by
running the UNMODIFIED reference torch backend under autograd: d loss / d input for a loss on image and depth.

Test infrastructure; runs only where the reference checkout is present (oracle/ref_harness.py).  Stored per fixture:
the scene, the upstream gradients, and d loss / d input for every differentiable input as torch autograd computes it
(float32, as the reference computes).

g9.  The scene is chosen in the regime where the torch backend's shading model coincides with the numpy backend's
(SURVEY.md section 8, row a-B / golden G9): up orthogonal to the view direction (the two camera bases then agree),
attenuation (1,0,0), coeffs (1,0,0) (no specular), ambient 0, every light in front of every surface (the per-light relu
is then the identity), planar primitives only.  Gradients through diffrend/torch/renderer.py:136-355.

g10 / g11.  The reference's full shading model (attenuation, specular coefficients, ambient, per-light relu, optional
double_sided / use_quartic): the gradients that `render(scene, shading='torch')` must reproduce, through
diffrend/torch/renderer.py:82-125,136-355.  ``build_scene`` is also the scene of the n1, c1 and v1 fixtures.
"""
import numpy as np

from oracle import ref_harness as R
from oracle.ref_harness import f32

H, W = 36, 48


def build_scene():
    return {
        "camera": {"viewport": [0, 0, 48, 36], "fovy": float(np.deg2rad(60.0)), "focal_length": 1.0,
                   "eye": [0.3, 1.0, 10.0, 1.0], "up": [0.0, 1.0, 0.0, 0.0], "at": [0.0, 0.0, 0.0, 1.0],
                   "near": 0.1, "far": 100.0},
        "lights": {"pos": f32([[2.5, 3.8, 9.5, 1], [-3.9, 1.3, 8.2, 1], [0.2, -4.7, 7.0, 1]]),
                   "color_idx": np.array([1, 2, 3]),
                   "attenuation": f32([[1, 0, 0], [0.4, 0.05, 0.002], [0.8, 0, 0.004]]),
                   "ambient": f32([0.03, 0.02, 0.025])},
        "colors": f32([[0, 0, 0], [.8, .3, .2], [.2, .7, .3], [.3, .3, .9]]),
        "materials": {"albedo": f32([[.5, .5, .5], [.9, .4, .2], [.2, .8, .6]]),
                      "coeffs": f32([[1.0, 0.0, 0.0], [0.7, 0.3, 6.0], [0.5, 0.5, 12.0]])},
        "objects": {
            "plane": {"pos": f32([[0, 0, -6, 1]]), "normal": f32([[0.1, -0.05, 1.5, 0]]), "material_idx": np.array([0])},
            "disk": {"pos": f32([[-2, 1, 1, 1], [1.5, -1, 2, 1], [0.5, 2, -1, 1]]),
                     "normal": f32([[0.2, 0.1, 1, 0], [-0.3, 0.2, 0.9, 0], [0, -0.4, 2, 0]]),
                     "radius": f32([1.6, 1.4, 2.2]), "material_idx": np.array([1, 2, 1])},
            "sphere": {"pos": f32([[-3.0, -2.0, 0.5, 1], [3.2, 1.8, -0.5, 1]]), "radius": f32([1.3, 1.1]),
                       "material_idx": np.array([2, 1])},
            "triangle": {"face": f32([[[-4, -3, -2, 1], [0, -3.5, -2.5, 1], [-2.5, 1, -1.5, 1]],
                                      [[1, 0, -3, 1], [4.5, -1, -3.5, 1], [3, 3, -2.5, 1]]]),
                         "normal": f32([[-0.05, 0.15, 1, 0], [0.1, 0.05, 1, 0]]), "material_idx": np.array([2, 0])},
        },
        "tonemap": {"type": "gamma", "gamma": 0.8},
    }


def build_scene_g9():
    """build_scene() in the numpy backend's regime: view direction along -z, lights in front of every surface, no
    spheres, no attenuation / ambient / coeffs."""
    sc = build_scene()
    sc["camera"]["eye"] = [0.0, 0.0, 10.0, 1.0]
    sc["lights"] = {"pos": f32([[0.5, 0.8, 10.5, 1], [-0.9, 0.3, 10.2, 1], [0.2, -0.7, 11.0, 1]]),
                    "color_idx": np.array([1, 2, 3])}
    del sc["materials"]["coeffs"], sc["objects"]["sphere"]
    return sc


ORTHO = {"proj_type": "ortho", "fovy": float(np.deg2rad(100.0)), "focal_length": 4.0}


def emit(name, camera=None, aux=False, **kw):
    """One image + depth (``aux``: + normal + pos) gradient fixture of ``build_scene()``; n1 is this with ``aux``."""
    if not R.wanted(name):
        return
    sc = build_scene()
    if camera:
        sc["camera"].update(camera)
    ups = R.upstream((H, W), aux=aux)
    tsc, leaves = R.torch_scene(sc)
    res = R.render(tsc, **kw)
    hit = res["depth"] <= sc["camera"]["far"]
    R.masked_loss(res, ups, hit).backward()
    R.write(name, R.pack_run(sc, ups, res, leaves, kw))
    print("hit fraction", float(hit.float().mean()))


def emit_g9(name):
    if not R.wanted(name):
        return
    sc = build_scene_g9()
    ups = R.upstream((H, W), rng=np.random.RandomState(99))
    tsc, leaves = R.torch_scene(sc)
    res = R.render(tsc)
    hit = res["depth"] < sc["camera"]["far"]
    R.masked_loss(res, ups, hit).backward()
    R.write(name, R.pack_run(sc, ups, res, leaves))
    print("hit fraction", float(hit.float().mean()))


def main():
    emit_g9("g9_torch_autograd")
    emit("g10_torch_autograd_phong")
    emit("g10_torch_autograd_phong_ds_quartic", double_sided=True, use_quartic=True)
    # orthographic projection (torch/utils.py:461-468): per-ray origins on the image plane, one direction; the
    # reference's ortho branch works while the image fits one 4096-pixel tile (48 x 36 does)
    emit("g11_torch_autograd_ortho", camera=ORTHO)
