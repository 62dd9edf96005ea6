"""bench.py's command line: the help text renders and the contract's flags exist (no GPU needed); on a GPU, what
--dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_renders_and_lists_the_contract_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    for flag in ("--gpus", "--steps", "--warmup", "--slabs", "--check", "--full", "--dump-outputs"):
        assert flag in out.stdout


def test_bench_refuses_to_run_without_a_gpu_or_with_a_wrong_world():
    import torch
    env = dict(os.environ, WORLD_SIZE="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                         timeout=300, env=env)
    assert out.returncode != 0 and "torch.distributed.run" in (out.stderr + out.stdout)
    if not torch.cuda.is_available():
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode != 0 and "needs a GPU" in (out.stderr + out.stdout)


def test_render_cli_refuses_torch_only_flags_on_other_backends():
    scene = os.path.join(ROOT, "assets", "scenes", "basic.json")
    for extra in (["--use", "np", "--shadow"], ["--use", "hip", "--double_sided"]):
        out = subprocess.run([sys.executable, "-m", "surf_renderer_amd.render_cli", "--scene", scene, *extra],
                             capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 2 and "--shading torch" in out.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_are_finite_and_equal_an_eager_render(tmp_path):
    """--dump-outputs of a small frame: every file finite, every pixel (a small frame is dumped whole) equal to an eager
    render of the same seeded scene -- depth 0 and hit 0 where nothing is hit (the library writes +inf there)."""
    import json
    import numpy as np
    import torch
    from surf_renderer_amd import renderer, synthetic
    from surf_renderer_amd.pipeline import slab_views
    W, H, M = 96, 64, 5000
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--prims", str(M),
                          "--width", str(W), "--height", str(H), "--steps", "3", "--warmup", "1", "--warmup-ms", "0",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, WORLD_SIZE="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    got = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in ("image", "depth", "hit", "pixel_index")}
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    np.testing.assert_array_equal(got["pixel_index"], np.arange(W * H, dtype=np.float64))

    scene = synthetic.disk_cloud_scene(M, W, H)
    buf = renderer.flatten_scene(scene, "cuda:0")
    slab = torch.empty((H, 4 * W), dtype=torch.float32, device="cuda:0")
    image, depth = slab_views(slab, W)
    renderer.render_buffers(buf, renderer.camera_struct(scene["camera"]), out=(image, depth, None))
    torch.cuda.synchronize()
    want_image, want_depth = image.cpu().numpy().reshape(-1, 3), depth.cpu().numpy().reshape(-1)
    hit = np.isfinite(want_depth)
    assert hit.any() and not hit.all()                  # both kinds of pixel are in the frame
    np.testing.assert_array_equal(got["hit"], hit.astype(np.float32))
    np.testing.assert_array_equal(got["depth"], np.where(hit, want_depth, np.float32(0)))
    np.testing.assert_array_equal(got["image"], want_image)
