"""float64 oracle of the image-metrics kernel's multi-scale and masked modes (csrc/metrics.hip: mmh_ms_ssim,
mmh_image_metrics_masked) and the cases tests/test_msssim_cpu.py, tests/test_msssim_gpu.py and tests/test_metrics_masked_gpu.py
share (plain module, no fixtures, no device).  Built on tests/_metrics_oracle.py, which is imported and left as it is.

MS-SSIM, per image and channel (include/mmhand_hip.h):
    level 0 = the pair mapped to [0, 1]; level l + 1 = F.avg_pool2d(level l, 2, padding=(H % 2, W % 2)): pooled pixel (i, j) =
    ((v00 + v01) + (v10 + v11)) * 0.25 over rows 2 i - ph, 2 i - ph + 1 and columns 2 j - pw, 2 j - pw + 1, zero outside;
    v_l = mean over the VALID interior (window / 2 <= y < H_l - window / 2, likewise x) of cs = (2 s_ab + C2) / (s_aa + s_bb + C2)
    for l < L - 1 and of the SSIM map for l = L - 1;  ms = mean over c of prod over l of max(v_l, 0) ** w_l.
In the valid interior the zero-padded moments of _metrics_oracle.ssim_map are those of a "valid" convolution: `maps` repeats that
function's tap-by-tap sums (and is held to it bit for bit by the CPU test) because the cs term needs the moments, not the map.

On the dyadic grid of _metrics_oracle (values k / 128 - 1, mapped to multiples of 1 / 256) every pooled value of four further
levels needs at most 8 + 2 * 4 = 16 fractional bits: fp32 pooling in the kernel's order is exact, so the device and this oracle
score the same levels and a level's value can be compared at the kernel's own per-pixel bar.

PROBE PAIRS (b = a except at a few pixels) make N_l (1 - v_l) a sum over the few valid pixels of level l whose window holds a
pooled probe; it is held to `affected_l * 1e-6`.  PERTURBED PAIRS (k_b = clip(k_a + e), |e| <= amp) keep every level's value
far from 0, where pow(v, 0.0448) is ill-conditioned; they carry the whole-value bound
    |ms - oracle| <= ms * sum_l w_l * 1e-6 / v_l        (first-order propagation of the per-level bar through the powers).
"""
import functools

import numpy as np
import torch

from tests import _metrics_oracle as M

C1, C2 = M.C1, M.C2
LEVEL_BAR = M.PIXEL_BAR                  # per affected pixel of a level, and per level value
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_FAULTS = ("pad_side", "divisor", "same_windows", "weights_reversed", "cs_last")
MASK_FAULTS = ("mask_shift_x", "mask_shift_y")
FLOOR = 0.5                              # every level value of a whole-value case stays above this (they are >= 0.92)


# ------------------------------------------------------------------------------------------------- maps and pooling
def maps(a01, b01, window):
    """(ssim_map, cs_map) float64 [B,C,H,W], zero padded: _metrics_oracle.ssim_map's moments, tap by tap in its order"""
    a, b = torch.as_tensor(a01, dtype=torch.float64), torch.as_tensor(b01, dtype=torch.float64)
    assert a.shape == b.shape and a.dim() == 4
    H, W = a.shape[2:]
    half = window // 2
    win = M.window2d(window)
    P = torch.stack([a, b, a * a, b * b, a * b]).reshape((-1, 1) + tuple(a.shape[2:]))
    P = torch.nn.functional.pad(P, (half, half, half, half))
    acc = torch.zeros((P.shape[0], 1, H, W), dtype=torch.float64)
    for i in range(window):
        for j in range(window):
            acc += P[:, :, i:i + H, j:j + W] * float(win[i, j])
    mu1, mu2, e11, e22, e12 = acc.reshape((5,) + tuple(a.shape))
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return ssim.numpy(), cs.numpy()


def valid(m, window):
    """the pixels whose whole window lies inside the image"""
    half = window // 2
    return m[..., half:m.shape[-2] - half, half:m.shape[-1] - half]


def pool(x, dtype=np.float64, fault=None):
    """One pyramid step in `dtype`, in the kernel's order.  fault "pad_side": an odd axis padded behind instead of in front;
    "divisor": divided by the number of in-image pixels instead of 4."""
    x = np.asarray(x, dtype=dtype)
    H, W = x.shape[-2:]
    ph, pw = H % 2, W % 2
    before = (0, 0) if fault == "pad_side" else (ph, pw)
    pad = [(0, 0)] * (x.ndim - 2) + [(before[0], ph - before[0]), (before[1], pw - before[1])]
    p = np.pad(x, pad)
    v00, v01, v10, v11 = p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]
    s = (v00 + v01) + (v10 + v11)
    assert s.dtype == dtype
    if fault == "divisor":
        n = np.pad(np.ones((H, W), dtype=dtype), pad[-2:])
        return (s / ((n[0::2, 0::2] + n[0::2, 1::2]) + (n[1::2, 0::2] + n[1::2, 1::2]))).astype(dtype)
    return s * dtype(0.25)


def level_sizes(H, W, levels):
    out = []
    for _ in range(levels):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def ms_ssim(a01, b01, window, weights, fault=None, pool_dtype=np.float64):
    """(ms [B], scales [B,C,L]) in float64; pool_dtype=np.float32 pools as the kernel does off the dyadic grid"""
    assert fault in (None,) + MS_FAULTS, fault
    w = np.asarray(weights, dtype=np.float64)
    L = len(w)
    a, b = np.asarray(a01, dtype=np.float64), np.asarray(b01, dtype=np.float64)
    scales = []
    for l in range(L):
        ssim, cs = maps(a, b, window)
        m = ssim if (l == L - 1 and fault != "cs_last") else cs
        m = m if fault == "same_windows" else valid(m, window)
        assert m.shape[-1] >= 1 and m.shape[-2] >= 1
        scales.append(m.sum(axis=(2, 3)) * (1.0 / float(m.shape[2] * m.shape[3])))
        if l + 1 < L:
            pf = fault if fault in ("pad_side", "divisor") else None
            a = pool(a.astype(pool_dtype), pool_dtype, pf).astype(np.float64)
            b = pool(b.astype(pool_dtype), pool_dtype, pf).astype(np.float64)
    scales = np.stack(scales, axis=2)
    ww = w[::-1] if fault == "weights_reversed" else w
    prod = np.ones(scales.shape[:2])
    for l in range(L):
        prod = prod * np.power(np.maximum(scales[:, :, l], 0.0), ww[l])
    return prod.sum(axis=1) / float(scales.shape[1]), scales


def whole_bound(ms, scales, weights):
    """|ms - oracle| allowed per image: ms * sum_l w_l * 1e-6 / (the case's smallest value of level l)"""
    w = np.asarray(weights, dtype=np.float64)
    return ms * (w * LEVEL_BAR / scales.min(axis=(0, 1))).sum()


# ------------------------------------------------------------------------------------------------- masked mode
def masked(a01, b01, mask, window, fault=None):
    """dict of float64 [B]: ssim_hand, l1_hand, mse_hand (sum * (1.0 / (C * count)), NaN at count 0) and count, from
    _metrics_oracle.ssim_map and .sums.  fault "mask_shift_x" / "_y": the mask read one pixel further (wrapping)."""
    assert fault in (None,) + MASK_FAULTS, fault
    a, b = np.asarray(a01, dtype=np.float64), np.asarray(b01, dtype=np.float64)
    m = (np.asarray(mask) != 0)
    assert m.shape == (a.shape[0],) + a.shape[2:]
    if fault is not None:
        m = np.roll(m, 1, axis=2 if fault == "mask_shift_x" else 1)
    m4 = m[:, None].astype(np.float64)
    count = m.reshape(m.shape[0], -1).sum(1).astype(np.float64)
    s_ssim = (M.ssim_map(a, b, window) * m4).sum(axis=(1, 2, 3))
    s1, s2, _, _ = M.sums(a * m4, b * m4)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (float(a.shape[1]) * count)
        return {"ssim_hand": s_ssim * inv, "l1_hand": s1 * inv, "mse_hand": s2 * inv, "count": count}


# ------------------------------------------------------------------------------------------------- perturbed pairs
AMPS = (16, 48)


def perturbed_pair(shape, seed, amps=AMPS):
    """grid-valued fp32 a and b with k_b = clip(k_a + e, 0, 255), e hashed from grid(..., 7001) into [-amp, amp]; image i
    takes amps[i % len(amps)]"""
    ka, h = M.grid(shape, seed, 7000), M.grid(shape, seed, 7001)
    kb = np.empty_like(ka)
    for i in range(shape[0]):
        amp = amps[i % len(amps)]
        kb[i] = np.clip(ka[i] + (h[i] % (2 * amp + 1)) - amp, 0, 255)
    return M.from_grid(ka), M.from_grid(kb)


# name: (shape, window, levels); "many": 17 x 16 = 272 tiles per plane at level 0, more than ms_ssim_final_kernel's 256 threads
WHOLE_CASES = {
    "five_levels": ((2, 3, 161, 176), 11, 5),
    "two_levels_w11": ((2, 1, 67, 45), 11, 2),
    "three_levels_w5": ((2, 3, 33, 33), 5, 3),
    "smallest": ((1, 1, 5, 6), 3, 2),
    "tall": ((1, 2, 513, 40), 3, 3),
    "many": ((1, 1, 520, 500), 3, 2),
}
WHOLE_SEEDS = {"five_levels": 1, "two_levels_w11": 1, "three_levels_w5": 1, "smallest": 1, "tall": 1, "many": 1}


@functools.lru_cache(maxsize=None)
def whole_case(name, seed=None):
    """a perturbed pair with the oracle's ms, scales and bound; computed once and shared, read-only"""
    shape, window, levels = WHOLE_CASES[name]
    seed = WHOLE_SEEDS[name] if seed is None else seed
    a, b = perturbed_pair(shape, seed)
    weights = MS_WEIGHTS[:levels]
    ms, scales = ms_ssim(M.mapped(a, "pm1"), M.mapped(b, "pm1"), window, weights)
    return dict(shape=shape, window=window, levels=levels, weights=weights, seed=seed, a=a, b=b, ms=ms, scales=scales,
                bound=whole_bound(ms, scales, weights))


# (case, fault) pairs a whole-value case is NOT held to, with the reason; the probe cases hold both faults
WHOLE_EXEMPT = {
    ("two_levels_w11", "divisor"): "row and column 0 of the 34 x 23 level are scaled alike in a and b, cs is invariant to a common "
                                   "scale but for C2, and a window of 11 sees them through its outermost taps: 2 to 4 bounds at "
                                   "seeds 1 .. 6",
}


def whole_fault_applies(name, case, fault):
    """cs_last never applies to a perturbed pair: e has zero mean, the local means of a and b agree to 1e-3 and the luminance
    factor that separates SSIM from cs is within 1e-6 of 1 (0.4 to 17 bounds over the cases).  The probe cases and the
    one-level test hold that fault."""
    if (name, fault) in WHOLE_EXEMPT or fault == "cs_last":
        return False
    odd = any(h % 2 or w % 2 for h, w in level_sizes(*case["shape"][2:], case["levels"])[:-1])
    return {"pad_side": odd, "divisor": odd, "same_windows": True, "weights_reversed": case["levels"] >= 2}[fault]


def whole_fault_effect(case, fault):
    """|ms_fault - ms| per image, on the oracle alone"""
    ms, _ = ms_ssim(M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1"), case["window"], case["weights"], fault=fault)
    return np.abs(ms - case["ms"])


# ------------------------------------------------------------------------------------------------- probe cases
def _probe_positions_67x45():
    """w = 5, L = 2: 67 x 45 (3 x 2 tiles, ragged) -> 34 x 23 (2 x 1 tiles, ragged); both axes odd: pooled row i takes rows
    2 i - 1, 2 i and pooled row / column 0 one zero."""
    return [(2, 2, "first valid row and column"), (64, 42, "last valid row and column"), (2, 42, "first row, last column"),
            (64, 2, "last row, first column"),
            (0, 0, "corner: outside the counted pixels of level 0, pooled with zeros"), (0, 44, "corner"), (66, 0, "corner"),
            (66, 44, "corner, ragged tile of both levels"),
            (0, 20, "row 0 of an odd level: pooled with the zero row"), (30, 0, "column 0 of an odd level"),
            # level-1 tile seam 31 | 32: pooled row 31 = rows 61, 62; 32 = rows 63, 64 (63 in level 0's tile row 1, 64 in tile row
            # 2, whose workgroup reads 63 from its halo); 33 = rows 65, 66
            (62, 10, "level-1 seam, upper side"), (63, 10, "level-1 seam: the halo row of the pooling workgroup"),
            (64, 10, "level-1 seam, lower side"), (65, 10, "level-1 seam, next pooled row"),
            (31, 31, "level-0 seam crossing"), (32, 32, "level-0 seam crossing"), (20, 21, "interior")]


def _probe_positions_131x70():
    """w = 3, L = 3: 131 x 70 (5 x 3 tiles) -> 66 x 35 (3 x 2) -> 33 x 18 (2 x 1): rows odd, even, odd; columns even, odd, even"""
    return [(1, 1, "first valid row and column"), (129, 68, "last valid row and column"),
            (0, 0, "corner"), (0, 69, "corner"), (130, 0, "corner"), (130, 69, "corner, ragged tile of every level"),
            (0, 33, "row 0 of an odd level"), (50, 0, "column 0: even at level 0, column 0 of the odd level 1"),
            (62, 40, "level-1 row seam"), (63, 40, "level-1 row seam: halo row"), (64, 40, "level-1 row seam"),
            (65, 40, "level-1 row seam"),
            (40, 62, "level-1 column seam 31 | 32: pooled column 31 = columns 62, 63"), (40, 63, "level-1 column seam"),
            (40, 64, "level-1 column seam: pooled column 32"), (40, 65, "level-1 column seam"),
            (63, 63, "level-1 seam crossing"), (64, 64, "level-1 seam crossing"),
            # level 2's seam 31 | 32 lies at level-1 rows 61 .. 64 (33 rows from 66: even, no shift) = level-0 rows 121 .. 128
            (125, 30, "level-2 row seam, upper side"), (127, 30, "level-2 row seam, lower side"), (100, 50, "interior")]


PROBE_SHAPES = {"67x45_w5_L2": ((67, 45), 5, 2, _probe_positions_67x45), "131x70_w3_L3": ((131, 70), 3, 3, _probe_positions_131x70)}
PROBE_SEEDS = {"67x45_w5_L2": 1, "131x70_w3_L3": 1}


def affected_levels(ka, kb, window, levels):
    """int [B, L]: per level the valid pixels whose window holds a pixel at which the pooled a and b differ (grid integers in)"""
    a, b = ka.astype(np.float64), kb.astype(np.float64)
    half = window // 2
    out = []
    for l in range(levels):
        diff = torch.from_numpy((a != b).astype(np.float64))
        hit = torch.nn.functional.max_pool2d(diff, window, stride=1, padding=half).numpy() > 0
        out.append(valid(hit, window).reshape(hit.shape[0], -1).sum(1))
        a, b = pool(a), pool(b)
    return np.stack(out, axis=1)


def level_S(scales, shape, window):
    """N_l (1 - v_l): float64 [B,C,L] from scales [B,C,L]"""
    n = np.array([(h - window + 1) * (w - window + 1) for h, w in level_sizes(shape[2], shape[3], scales.shape[2])], dtype=np.float64)
    return n[None, None, :] * (1.0 - scales)


@functools.lru_cache(maxsize=None)
def probe_case(name, seed=None):
    """one image per probe position (C = 1): a, b, the oracle's scales, S = N_l (1 - v_l) [B,L] and affected [B,L]"""
    (H, W), window, levels, positions = PROBE_SHAPES[name]
    pos = positions()
    assert len({(y, x) for y, x, _ in pos}) == len(pos)
    seed = PROBE_SEEDS[name] if seed is None else seed
    shape = (len(pos), 1, H, W)
    ka = M.grid(shape, seed)
    kb = ka.copy()
    for i, (y, x, _) in enumerate(pos):
        kb[i, 0, y, x] = (ka[i, 0, y, x] + 128) % 256
    a, b = M.from_grid(ka), M.from_grid(kb)
    weights = MS_WEIGHTS[:levels]
    ms, scales = ms_ssim(M.mapped(a, "pm1"), M.mapped(b, "pm1"), window, weights)
    return dict(shape=shape, window=window, levels=levels, weights=weights, seed=seed, why=[w for _, _, w in pos], a=a, b=b,
                ms=ms, scales=scales, S=level_S(scales, shape, window)[:, 0], affected=affected_levels(ka, kb, window, levels))


def probe_fault_effect(case, fault):
    """max over the levels of |S_fault - S| / (affected * 1e-6) per image: how many bars the planted fault moves the image.
    A level the fault empties of affected pixels counts with one pixel's bar."""
    _, scales = ms_ssim(M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1"), case["window"], case["weights"], fault=fault)
    Sf = level_S(scales, case["shape"], case["window"])[:, 0]      # the test multiplies by the valid count whatever the kernel did
    return (np.abs(Sf - case["S"]) / (np.maximum(case["affected"], 1) * LEVEL_BAR)).max(axis=1)


MEAN_GAP = 0.004


def last_level_mean_gap(case):
    """float64 [B]: the largest |mu_a - mu_b| over the last level's valid pixels.  SSIM = cs * luminance and luminance =
    1 - (mu_a - mu_b)^2 / (mu_a^2 + mu_b^2 + C1): a kernel that takes cs at the last level is visible only where the local
    means differ.  At a gap of MEAN_GAP and means up to 0.75 that is (0.004)^2 / (2 * 0.75^2) = 1.4e-5, fourteen bars of one
    pixel; a probe that the last level's only affected pixel sees through its corner tap (67 x 45, w = 5: weight 0.0144 on a
    pooled difference of 1 / 8) stays below it, and the fault does not apply to that image."""
    a, b = M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1")
    for _ in range(case["levels"] - 1):
        a, b = pool(a), pool(b)
    win = torch.from_numpy(M.window2d(case["window"]))[None, None]
    gap = torch.nn.functional.conv2d(torch.from_numpy(a - b).reshape((-1, 1) + a.shape[2:]), win).abs()
    return gap.reshape(a.shape[0], -1).max(dim=1).values.numpy()


def probe_fault_applies(case, fault):
    """bool [B]: does the planted fault change what this image's probe contributes"""
    B, _, H, W = case["shape"]
    sizes = level_sizes(H, W, case["levels"])
    odd = any(h % 2 or w % 2 for h, w in sizes[:-1])
    if fault == "pad_side":
        return np.full(B, odd)
    if fault == "cs_last":
        return last_level_mean_gap(case) >= MEAN_GAP
    if fault == "same_windows":
        return np.full(B, True)          # every level's mean runs over H_l W_l pixels instead of the valid ones
    if fault == "divisor":               # only a pooled pixel of row / column 0 on an odd axis has a different divisor
        out = np.zeros(B, dtype=bool)
        ka = (case["a"].numpy().astype(np.float64) != case["b"].numpy().astype(np.float64))
        for l, (h, w) in enumerate(sizes[:-1]):
            if h % 2:
                out |= ka[:, 0, 0, :].any(axis=1)
            if w % 2:
                out |= ka[:, 0, :, 0].any(axis=1)
            ka = pool(ka.astype(np.float64)) != 0
        return out
    raise AssertionError(fault)


# ------------------------------------------------------------------------------------------------- masked cases
def one_pixel_masks(name, window):
    """(positions, masks uint8 [P,H,W]) for _metrics_oracle.positions_67x45 / positions_33x33: mask i is the one pixel i"""
    (H, W), positions = M.SINGLE_SHAPES[name]
    pos = positions(window)
    masks = np.zeros((len(pos), H, W), dtype=np.uint8)
    for i, (y, x, _) in enumerate(pos):
        masks[i, y, x] = 1
    return pos, masks


MASK_SEEDS = {("67x45", 3): 1, ("67x45", 5): 1, ("67x45", 11): 1, ("67x45", 15): 1, ("33x33", 3): 1, ("33x33", 5): 1,
              ("33x33", 11): 1, ("33x33", 15): 1}


@functools.lru_cache(maxsize=None)
def one_pixel_case(name, window, seed=None):
    """independent grid pairs, one image per position of the shape's list, each with the one-pixel mask of its position"""
    pos, masks = one_pixel_masks(name, window)
    (H, W), _ = M.SINGLE_SHAPES[name]
    seed = MASK_SEEDS[name, window] if seed is None else seed
    a, b = M.grid_pair((len(pos), 1, H, W), seed)
    ref = masked(M.mapped(a, "pm1"), M.mapped(b, "pm1"), masks, window)
    return dict(a=a, b=b, masks=masks, window=window, seed=seed, why=[w for _, _, w in pos], ref=ref)


def mask_fault_effect(case, fault):
    """|ssim_hand_fault - ssim_hand| per image, on the oracle alone"""
    f = masked(M.mapped(case["a"], "pm1"), M.mapped(case["b"], "pm1"), case["masks"], case["window"], fault=fault)
    return np.abs(f["ssim_hand"] - case["ref"]["ssim_hand"])


def clear_caches():
    for fn in (whole_case, probe_case, one_pixel_case):
        fn.cache_clear()
