"""Generate tests/golden/n1_*.npz: gradients of a loss on ALL FOUR outputs of the reference torch backend -- image,
depth, normal and pos -- from the UNMODIFIED reference running under autograd on the CPU, the way
oracle/golden_g9_g11.py produces the image + depth fixtures (same scene, same upstream image / depth gradients):

    loss = sum image * g_i + sum_hit depth * g_d + sum_hit normal . g_n + sum_hit pos . g_p

with the three per-pixel terms masked by torch.where(hit, ., 0): the hip backend ignores the upstream gradients of
misses (the reference differentiates object 0's intersection there).

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by
hand -- no test reads the reference.  Stored: the scene, the four upstream gradients, ref/{image, depth,
nearest, normal, pos} and d loss / d input for every differentiable input (float32, as the reference computes).
"""
from oracle.golden_g9_g11 import ORTHO, emit


def main():
    emit("n1_aux_grad_phong", aux=True)
    emit("n1_aux_grad_phong_ds_quartic", aux=True, double_sided=True, use_quartic=True)
    # orthographic: per-pixel ray origins on the image plane (camera as in g11_torch_autograd_ortho)
    emit("n1_aux_grad_ortho", aux=True, camera=ORTHO)
