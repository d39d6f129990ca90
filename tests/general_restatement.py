"""Torch restatement of the general attention entry points (et_epipolar_forward_general / et_epipolar_backward_general_ga) at the
level of their C ABI, written from the description in include/epipolar_amd.h and the line references into the reference's
epipolar.py given there -- not from the kernels.  `Epipolar._attend_general_chunk` restates the same branches one level up, where
the similarity and the value map come from one feature map: it cannot reach c_sim != c_val or c_val > 512.  This one takes the
three maps the entry points take, in whatever dtype they come (the tests use float64), and autograd gives the gradients.

    out, attn, corr_pos, idx = attend(spec, q, map_sim, map_val, locs, prior, flags, absorb=None, idx=None)

spec: ops.LayerSpec (H, W, K, softmax_scale, softmax_enabled, align_corners, correct_normalize are read); q, map_sim (N,H,W,Cs) and
map_val (N,H,W,Cv) channels last; locs (K,N,H,W,2): ops.sample_locs(spec, cam) cast to the maps' dtype (those locations are pinned
bit-equal to the reference's by tests/test_gpu_parity.py); prior (N,K',H,W) or None; flags: dict of bools pooling, prior_mul,
cosine, attention_max, sim_prior (absent: False).  Returns out (N,H,W,Cv), attn (N,K',H,W), corr_pos (N,H,W,2) in the dtype of
`locs` and the arg-max it used, (N,H,W): the first maximum of attn over K' -- or the `idx` it was given (see near_maxima).

`absorb`: a dtype in which the sum of a MASKED similarity and its additive prior is rounded (None: not at all).  The reference and
the kernels add in float32, where -1e10 absorbs any prior below 512 (one ulp of 1e10 is 1024), so an all-masked pixel keeps its
uniform attention; in float64 the same expression keeps the prior, and the soft-max of such a pixel becomes the soft-max of the
priors.  This is the one place where the float32 of the reference is part of what it computes and not of how accurately."""
import torch
import torch.nn.functional as F


def sample(spec, m, locs, pooling):
    """epipolar.py:199 / :210 (+ POOLING :200-202, :211-213): (N,H,W,C) -> (N,K',C,H,W), the per-channel maximum of samples k and
    k + K/2 under pooling."""
    K, (N, H, W, C) = locs.shape[0], m.shape
    grid = locs.permute(1, 0, 2, 3, 4).reshape(N, K * H, W, 2)
    s = F.grid_sample(m.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=bool(spec.align_corners))
    s = s.view(N, C, K, H, W).permute(0, 2, 1, 3, 4)
    if pooling:
        s = s.reshape(N, 2, K // 2, C, H, W).max(1)[0]
    return s


def first_argmax(a):
    """torch.argmax's documented tie rule made explicit: the lowest index among the maxima of dim 1."""
    ks = torch.arange(a.shape[1], device=a.device).view(1, -1, 1, 1)
    return torch.where(a == a.max(1, keepdim=True)[0], ks, a.shape[1]).min(1)[0]


def de_normalize(spec, pos):
    """vision/multiview.py:39-57 in the dtype of `pos` (..., 2)."""
    H, W = spec.H, spec.W
    if spec.correct_normalize:
        return torch.stack([(pos[..., 0] + 1) * (W - 1) / 2, (pos[..., 1] + 1) * (H - 1) / 2], -1)
    return torch.stack([(pos[..., 0] + 1) * W / 2 - 0.5, (pos[..., 1] + 1) * H / 2 - 0.5], -1)


def near_maxima(attn, tie):
    """(N,K',H,W) bool: the samples whose weight is within tie * max(1, |max|) of the pixel's largest.  Where the samples of a
    pixel see one source pixel only (beyond the outermost pixel centres in both directions, zero padding) their sampled vectors
    are multiples of one another and the cosine similarities are equal -- to the last bit or two in float64 (tie = 1e-12).  No
    arithmetic separates such samples: under ATTENTION max, which gathers the arg-max sample, `attend(idx=...)` evaluates the
    operator at whichever member of that set an implementation took."""
    top = attn.amax(1, keepdim=True)
    return attn >= top - tie * top.abs().clamp_min(1.0)


def attend(spec, q, map_sim, map_val, locs, prior=None, flags=None, absorb=None, idx=None):
    fl = dict(pooling=False, prior_mul=False, cosine=False, attention_max=False, sim_prior=False)
    fl.update(flags or {})
    N, H, W = q.shape[:3]
    s2 = sample(spec, map_val, locs, fl["pooling"])
    Ks = s2.shape[1]
    if fl["sim_prior"]:                                                     # epipolar.py:288-289: the table is the attention
        sim = prior
    else:
        s1 = sample(spec, map_sim, locs, fl["pooling"])
        qe = q.permute(0, 3, 1, 2).unsqueeze(1)                             # (N,1,Cs,H,W)
        if fl["cosine"] or fl["attention_max"]:                             # :282-286, :290-293
            sim = F.cosine_similarity(qe.expand(-1, Ks, -1, -1, -1), s1, 2, eps=1e-8)
        else:
            sim = (s1 * qe).sum(2)                                          # :294-295
        if not fl["attention_max"]:                                         # (ATTENTION max: the raw cosine, no mask / soft-max)
            masked = sim == 0
            sim = sim.masked_fill(masked, -1e10)                            # :298
            if prior is not None and not fl["prior_mul"]:
                sim = sim + prior                                           # :300-301
                if absorb is not None:      # (the value rounded, the gradient that of the sum: what float32 autograd gives)
                    sim = torch.where(masked, sim.detach().to(absorb).to(sim.dtype) + (sim - sim.detach()), sim)
            if spec.softmax_enabled:
                sim = F.softmax(sim * spec.softmax_scale, 1)                # :303-307
                if prior is not None and fl["prior_mul"]:
                    sim = sim * prior                                       # :308-309
            else:
                sim = sim / Ks                                              # :310-311
    if idx is None:
        idx = first_argmax(sim.detach())                                    # :225 / :237
    # the location of sample idx of the UNPOOLED list (:239 indexes sample_locs with the pooled index)
    pos = torch.gather(locs.permute(1, 0, 2, 3, 4), 1, idx.view(N, 1, H, W, 1).expand(-1, -1, -1, -1, 2)).squeeze(1)
    if fl["attention_max"]:                                                 # :232-235: the arg-max sample's values
        out = torch.gather(s2, 1, idx.view(N, 1, 1, H, W).expand(-1, -1, s2.shape[2], -1, -1)).squeeze(1)
    else:
        out = (s2 * sim.unsqueeze(2)).sum(1)                                # :243
    return out.permute(0, 2, 3, 1), sim, de_normalize(spec, pos), idx
