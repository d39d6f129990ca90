"""What KEYPOINT.TRIANGULATION rpsm needs besides the kernels (ops.rpsm): the skeleton, the limb lengths and the crop transform of
the reference's pictorial structure model (modeling/pictorial_cuda.py, modeling/layers/body.py, data/transforms/image.py)."""
from __future__ import annotations

import torch

# modeling/layers/body.py:29-35: root, rhip, rkne, rank, lhip, lkne, lank, belly, neck, nose, head, lsho, lelb, lwri, rsho, relb,
# rwri -- every joint's parent, the root has -1
H36M_PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)


def limb_lengths(pose: torch.Tensor, parent=H36M_PARENT) -> torch.Tensor:
    """compute_limb_length (body.py:9-19) for a batch: pose (..., J, 3) -> (..., J - 1), limb e = the distance between the e-th
    non-root joint (ascending) and its parent: the order ops.rpsm takes."""
    child = [j for j, p in enumerate(parent) if p >= 0]
    idx_c = torch.tensor(child, device=pose.device)
    idx_p = torch.tensor([parent[j] for j in child], device=pose.device)
    return (pose.index_select(-2, idx_p) - pose.index_select(-2, idx_c)).norm(dim=-1)


def crop_transform(center: torch.Tensor, scale: torch.Tensor, image_size) -> torch.Tensor:
    """get_affine_transform(center, scale, 0, image_size) (data/transforms/image.py:226-258) in closed form: the reference solves
    the three-point system center -> (w/2, h/2), center - (0, 100 scale_x) -> (w/2, h/2 - w/2) and their perpendicular third points,
    which for rot = 0 is the uniform scaling a = w / (200 scale_x) about the centre.  center (..., 2), scale (..., 2) or (...,)
    -> (..., 2, 3) float32."""
    center = center.to(torch.float32)
    scale = scale.to(device=center.device, dtype=torch.float32)
    sx = scale[..., 0] if scale.dim() == center.dim() else scale
    w, h = float(image_size[0]), float(image_size[1])
    a = w / (200.0 * sx)
    zero = torch.zeros_like(a)
    return torch.stack([torch.stack([a, zero, w / 2 - a * center[..., 0]], -1),
                        torch.stack([zero, a, h / 2 - a * center[..., 1]], -1)], -2)
