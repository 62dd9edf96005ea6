"""Everything the mesh-sampling kernels index by is refused on the host, with a ValueError, before a GPU is touched:
this file runs where there is none (gpu_device would raise RuntimeError first if a check came too late)."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import mesh_sampling as ms
from surf_renderer_amd import mesh_topology, sample_mesh_batched, uniform_sample_mesh

V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32)
F = np.array([[0, 1, 2], [1, 3, 2]])
U = np.array([[0.1, 0.2, 0.3], [0.7, 0.5, 0.9]])
VB, UB = np.stack([V, V + 1]), np.stack([U, U])


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_the_names_are_exported_lazily():
    import surf_renderer_amd
    for name in ("uniform_sample_mesh", "sample_mesh_batched", "mesh_topology", "MeshSamples"):
        assert name in surf_renderer_amd.__all__ and getattr(surf_renderer_amd, name) is getattr(ms, name)


def test_shapes_are_refused():
    refused("v is", sample_mesh_batched, V[:, :2], F, U)
    refused("v is", sample_mesh_batched, V[None, None], F, U)
    refused("floating", sample_mesh_batched, V.astype(np.int32), F, U)
    refused("f is", sample_mesh_batched, V, F[:, :2], U)
    refused("f is", sample_mesh_batched, V, F.reshape(-1), U)
    refused("integer", sample_mesh_batched, V, F.astype(np.float32), U)
    refused("f is missing", sample_mesh_batched, V, None, U)
    refused("uniforms is", sample_mesh_batched, V, F, U[:, :2])
    refused("uniforms is", sample_mesh_batched, V, F, UB)                  # a batch of uniforms for one mesh
    refused("uniforms is", sample_mesh_batched, VB, F, U)
    refused("uniforms is", sample_mesh_batched, VB, F, np.stack([U, U, U]))
    refused("views", sample_mesh_batched, VB, np.stack([F, F, F]), UB)     # three face lists for two views
    refused("views", sample_mesh_batched, V, np.stack([F]), U)             # per-view faces for an unbatched mesh
    refused("eye is", sample_mesh_batched, VB, F, UB, eye=[0.0, 0.0])
    refused("eye is", sample_mesh_batched, VB, F, UB, eye=np.zeros((3, 3)))
    refused("eye is", sample_mesh_batched, V, F, U, eye=np.zeros((1, 3)))


def test_sizes_are_refused():
    refused("views", sample_mesh_batched, np.zeros((0, 4, 3), np.float32), F, np.zeros((0, 2, 3)))
    refused("views", sample_mesh_batched, torch.zeros(1, 4, 3).expand(65536, 4, 3), F, torch.zeros(1, 1, 3).expand(65536, 1, 3))
    refused("vertices", sample_mesh_batched, np.zeros((0, 3), np.float32), F, U)
    refused("vertices", sample_mesh_batched, torch.zeros(1, 3).expand((1 << 24) + 1, 3), F, U)
    refused("faces", sample_mesh_batched, V, np.zeros((0, 3), np.int64), U)
    refused("faces", sample_mesh_batched, V, torch.zeros(1, 3, dtype=torch.int64).expand((1 << 24) + 1, 3), U)
    refused("samples", sample_mesh_batched, V, F, np.zeros((0, 3)))
    refused("samples", sample_mesh_batched, V, F, torch.zeros(1, 3, dtype=torch.float64).expand((1 << 24) + 1, 3))


def test_uniforms_outside_the_unit_interval_are_refused():
    for bad in (1.0, -1e-9, 2.5, float("nan"), float("inf")):
        for col in range(3):
            u = U.copy()
            u[1, col] = bad
            refused(r"outside \[0, 1\)", sample_mesh_batched, V, F, u)
    refused(r"outside \[0, 1\)", uniform_sample_mesh, {"v": V, "f": F}, 2, uniforms=np.array([[0.5, 0.5, 1.0]] * 2))


def test_face_indices_outside_the_vertices_are_refused():
    for bad in (-1, 4, 1 << 40):
        f = F.copy()
        f[1, 2] = bad
        refused("entries in", sample_mesh_batched, V, f, U)
        refused("entries in", mesh_topology, f, 4)
        refused("entries in", uniform_sample_mesh, {"v": V, "f": f}, 2)
    refused("entries in", mesh_topology, torch.tensor(F), 3)
    refused("vertices", mesh_topology, F, 0)
    refused("f is", mesh_topology, F.reshape(1, 1, 2, 3), 4)


def test_a_topology_of_another_mesh_is_refused():
    topo = ms.MeshTopology(torch.tensor(F, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), 4)
    assert topo.n_faces == 2 and topo.n_views is None
    refused("topology was made for 4 vertices", sample_mesh_batched, np.zeros((5, 3), np.float32), None, U, topology=topo)
    refused("topology was made for", sample_mesh_batched, V, F[:1], U, topology=topo)
    refused("topology is a", sample_mesh_batched, V, F, U, topology=(F, 4))
    per_view = ms.MeshTopology(torch.tensor(np.stack([F, F, F]), dtype=torch.int32), torch.zeros((3, 6), dtype=torch.int32), 4)
    assert per_view.n_views == 3
    refused("views", sample_mesh_batched, VB, None, UB, topology=per_view)


def test_the_references_call_refuses_what_it_does_not_honour():
    refused("'a'", uniform_sample_mesh, {"v": V, "f": F, "a": np.ones(2)}, 2)
    refused("'fn'", uniform_sample_mesh, {"v": V, "f": F, "fn": np.ones((2, 3))}, 2)
    refused("needs 'v' and 'f'", uniform_sample_mesh, {"v": V}, 2)
    refused(r"obj\['v'\] is", uniform_sample_mesh, {"v": VB, "f": F}, 2)
    refused(r"obj\['f'\] is", uniform_sample_mesh, {"v": V, "f": np.stack([F])}, 2)
    for bad in (0, -3, 2.5, True, None):
        refused("num_samples", uniform_sample_mesh, {"v": V, "f": F}, bad)
    refused("no 'eye'", uniform_sample_mesh, {"v": V, "f": F}, 2, camera={"at": [0, 0, 0]})
    refused("uniforms is", uniform_sample_mesh, {"v": V, "f": F}, 3, uniforms=U)


def test_a_refused_call_leaves_the_generator_where_it_was():
    rng = np.random.RandomState(3)
    before = rng.get_state()[1].copy()
    f = F.copy()
    f[0, 0] = 9
    refused("entries in", uniform_sample_mesh, {"v": V, "f": f}, 5, rng=rng)
    assert np.array_equal(rng.get_state()[1], before)
