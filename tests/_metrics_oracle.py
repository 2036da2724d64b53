"""Per-pixel float64 oracle of the image-metrics kernel (csrc/metrics.hip) and the probe cases of
tests/test_metrics_local_gpu.py (plain module, no fixtures, no device).

The kernel returns one mean per image, and a mean hides a wrong pixel: at 3 x 256 x 256 one SSIM pixel that is off by 0.1
moves the mean by 5e-7.  A PROBE PAIR makes the mean local again: b equals a except at a few listed pixels, so the SSIM
map is exactly 1 wherever the window holds no probe - in float64 here, and on the device too (the kernel's a and b paths
are the same instructions and every shift pixel a pixel uses lies inside its own window) - and

    S = C H W (1 - ssim)  =  sum of (1 - map) over the `affected` pixels alone.

S is compared with `affected * 1e-6`: the documented 1e-6 of mmhand_amd/metrics.py per pixel, not per image.  A probe that
is read one pixel off, a border that is padded with anything but zero or a tap that is left out moves S by 1e-2 and more
(planted on the oracle by `fault=`; tests/test_metrics_local_cpu.py holds every case to ten times its bar).

The values live on the grid k / 128 - 1, k = 0 .. 255 (exact in fp32, bf16 and fp16): the kernel's map fma(x, .5, .5) is
then an exact multiple of 1/256, every |a - b| a multiple of 2^-8 and every (a - b)^2 a multiple of 2^-16, so the float64
sums behind L1 and MSE are exact in any order and the kernel's means must equal `sum * (1.0 / N)` bit for bit.

The case lists are here so that the CPU test checks the sensitivity and the caps of exactly the cases the device runs.
Every probe position is there for one place in csrc/metrics.hip; the line numbers are those of the file as of this test
(the function names are given beside them) - when the kernel changes, this is the list to read again.
"""
import functools

import numpy as np
import torch

from tests._hpe_oracle import hashed

C1, C2 = 0.01 ** 2, 0.03 ** 2
MT, MTPB = 32, 256                      # metrics.hip:34-35: output tile edge, threads per workgroup
PIXEL_BAR = 1e-6                        # metrics.py: "within 1e-6 of that formula evaluated in float64", per affected pixel
UNIT_L1, UNIT_SE = 2.0 ** -8, 2.0 ** -16
FAULTS = ("replicate", "shift_col", "shift_row", "drop_tap")


# ------------------------------------------------------------------------------------------------- the kernel's inputs
def _ranges():
    from mmhand_amd.metrics import RANGES
    return RANGES


def mapped(t, range):
    """What the kernel holds of `t` after load_halos_t (metrics.hip:62-63): the value read in its own dtype, converted to
    fp32, then ONE fp32 fma(x, scale, offset) with the fp32 roundings of RANGES[range].  float64 numpy [B,C,H,W];
    "u8_bgr_hwc" takes uint8 [B,H,W,3] in B,G,R order and returns R,G,B planes.  (x * scale + offset is exact in float64
    for every fp32 x that is not tiny against offset - 24 x 24 significand bits - so rounding it once to fp32 is the fma.)"""
    scale, offset = (np.float64(np.float32(v)) for v in _ranges()[range])
    t = t.detach().cpu()
    if range == "u8_bgr_hwc":
        assert t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3, (t.dtype, tuple(t.shape))
        x = t.flip(-1).permute(0, 3, 1, 2).to(torch.float32)
    else:
        assert t.dtype in (torch.float32, torch.bfloat16, torch.float16) and t.dim() == 4, (t.dtype, tuple(t.shape))
        x = t.to(torch.float32)
    x = x.contiguous().numpy().astype(np.float64)
    return (x * scale + offset).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------- SSIM, per pixel
def window2d(window):
    """pytorch_ssim.create_window: the fp32 outer product of the fp32 taps"""
    from mmhand_amd.metrics import gaussian_taps
    g = gaussian_taps(window)
    w = np.outer(g, g)
    assert w.dtype == np.float32
    return w.astype(np.float64)


def ssim_map(a01, b01, window, fault=None):
    """The reference's formula (pytorch_ssim._ssim) per pixel in float64: float64 [B,C,H,W] in, the map [B,C,H,W] out.
    The five moments are sums of window[i, j] * padded[y + i, x + j] added tap by tap in one fixed order, so a pixel's
    value is a function of its own window alone: where a and b agree on a window the map is 1.0 exactly.

    fault (planted errors, for the sensitivity test only): "replicate" pads with the border pixel instead of zero;
    "drop_tap" leaves out the window column right of the centre (one product of the horizontal pass)."""
    assert fault in (None, "replicate", "drop_tap"), fault
    a, b = torch.as_tensor(a01, dtype=torch.float64), torch.as_tensor(b01, dtype=torch.float64)
    assert a.shape == b.shape and a.dim() == 4
    H, W = a.shape[2:]
    half = window // 2
    win = window2d(window)
    if fault == "drop_tap":
        win[:, half + 1] = 0.0
    P = torch.stack([a, b, a * a, b * b, a * b])
    P = P.reshape((-1, 1) + tuple(a.shape[2:]))
    if fault == "replicate":
        for _ in range(half):            # one pixel at a time: also legal where the image is smaller than the pad
            P = torch.nn.functional.pad(P, (1, 1, 1, 1), mode="replicate")
    else:
        P = torch.nn.functional.pad(P, (half, half, half, half))
    acc = torch.zeros((P.shape[0], 1, H, W), dtype=torch.float64)
    for i in range(window):
        for j in range(window):
            if win[i, j] != 0.0:
                acc += P[:, :, i:i + H, j:j + W] * float(win[i, j])        # product, then sum: two roundings, no fma
    mu1, mu2, e11, e22, e12 = acc.reshape((5,) + tuple(a.shape))
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return m.numpy()


def one_minus_sum(a01, b01, window, fault=None):
    """sum over an image of (1 - map): float64 [B]"""
    return (1.0 - ssim_map(a01, b01, window, fault)).sum(axis=(1, 2, 3))


def sums(a01, b01):
    """(sum |a - b|, sum (a - b)^2, l1, mse) per image in float64; the means exactly as the kernel takes them
    (image_metrics_final_kernel: sum * inv_count, inv_count = 1.0 / ((double)C * H * W))"""
    d = np.asarray(a01, dtype=np.float64) - np.asarray(b01, dtype=np.float64)
    n = d.shape[1] * d.shape[2] * d.shape[3]
    inv = 1.0 / float(n)
    s1, s2 = np.abs(d).sum(axis=(1, 2, 3)), (d * d).sum(axis=(1, 2, 3))
    return s1, s2, s1 * inv, s2 * inv


def check_caps(a01, b01):
    """The conditions that make the L1 / MSE sums exact in ANY order: every term an integer number of units, every sum
    (hence every partial sum of non-negative terms) under 2^36 units, far inside float64's 53 bits."""
    d = np.asarray(a01, dtype=np.float64) - np.asarray(b01, dtype=np.float64)
    u1, u2 = np.abs(d) / UNIT_L1, (d * d) / UNIT_SE
    assert np.array_equal(u1, np.rint(u1)) and np.array_equal(u2, np.rint(u2)), "a value is off the dyadic grid"
    i1 = u1.astype(np.int64).reshape(d.shape[0], -1).sum(1)
    i2 = u2.astype(np.int64).reshape(d.shape[0], -1).sum(1)
    assert int(i1.max()) < 2 ** 36 and int(i2.max()) < 2 ** 36, (i1.max(), i2.max())
    s1, s2, _, _ = sums(a01, b01)
    assert np.array_equal(s1, i1.astype(np.float64) * UNIT_L1) and np.array_equal(s2, i2.astype(np.float64) * UNIT_SE)
    return i1, i2


# ------------------------------------------------------------------------------------------------- grid values, probes
def grid(shape, seed, tensor_index=7000):
    """integers k in 0 .. 255 from the project's hash generator (tests/_hpe_oracle.hashed); the value is k / 128 - 1"""
    n = int(np.prod(shape))
    k = np.floor((hashed(tensor_index, n, seed) + 1.0) * 128.0).astype(np.int64)
    assert k.min() >= 0 and k.max() <= 255
    return k.reshape(shape)


def from_grid(k):
    return torch.from_numpy((k.astype(np.float64) / 128.0 - 1.0).astype(np.float32))


def grid_pair(shape, seed):
    """two independent grid-valued fp32 tensors (the small-image cases: no probe)"""
    return from_grid(grid(shape, seed, 7000)), from_grid(grid(shape, seed, 7001))


def affected_mask(shape, probes, window):
    """bool [B,C,H,W]: the output pixels whose window contains a probe"""
    B, C, H, W = shape
    half = window // 2
    m = np.zeros(shape, dtype=bool)
    for (b, c, y, x) in probes:
        assert 0 <= b < B and 0 <= c < C and 0 <= y < H and 0 <= x < W, ((b, c, y, x), shape)
        m[b, c, max(0, y - half):y + half + 1, max(0, x - half):x + half + 1] = True
    return m


def probe_pair(shape, probes, seed, window):
    """a: grid values; b = a except at the (b, c, y, x) probes, which move by half the range (k -> (k + 128) mod 256, so
    |a01 - b01| = 1/2 exactly).  Returns fp32 torch tensors a, b and `affected` [B]: per image, the number of output
    pixels whose window contains a probe."""
    assert len(set(probes)) == len(probes)
    k = grid(shape, seed)
    kb = k.copy()
    for p in probes:
        kb[p] = (k[p] + 128) % 256
    return from_grid(k), from_grid(kb), affected_mask(shape, probes, window).reshape(shape[0], -1).sum(1)


def shifted(probes, shape, axis):
    """the planted read-one-pixel-off fault: every probe one column ("col") or one row ("row") further, towards the inside
    where it sits on the last one.  None where the image has no second column / row."""
    B, C, H, W = shape
    if (W if axis == "col" else H) < 2:
        return None
    out = []
    for (b, c, y, x) in probes:
        if axis == "col":
            x = x + 1 if x + 1 < W else x - 1
        else:
            y = y + 1 if y + 1 < H else y - 1
        out.append((b, c, y, x))
    return out


def window_leaves_image(probes, shape, window):
    """per image: does some probe's own window reach past a border (the padding fault applies)"""
    B, C, H, W = shape
    half = window // 2
    out = np.zeros(B, dtype=bool)
    for (b, c, y, x) in probes:
        if y < half or x < half or y + half >= H or x + half >= W:
            out[b] = True
    return out


def fault_effects(case):
    """{fault: (|S_fault - S| per image, applies per image)} of one probe case, on the oracle alone"""
    shape, probes, w = case["shape"], case["probes"], case["window"]
    a01, b01 = mapped(case["a"], "pm1"), mapped(case["b"], "pm1")
    out = {}
    for axis in ("col", "row"):
        moved = shifted(probes, shape, axis)
        applies = np.full(shape[0], moved is not None)
        if moved is None:
            out["shift_" + axis] = (np.zeros(shape[0]), applies)
            continue
        _, b2, _ = probe_pair(shape, moved, case["seed"], w)
        out["shift_" + axis] = (np.abs(one_minus_sum(a01, mapped(b2, "pm1"), w) - case["S"]), applies)
    out["drop_tap"] = (np.abs(one_minus_sum(a01, b01, w, fault="drop_tap") - case["S"]), np.full(shape[0], True))
    out["replicate"] = (np.abs(one_minus_sum(a01, b01, w, fault="replicate") - case["S"]),
                        window_leaves_image(probes, shape, w))
    return out


# ------------------------------------------------------------------------------------------------- the probe cases
WINDOWS = (3, 5, 11, 15)


def last_round_pixel(window):
    """Image coordinates (tile 0) of a halo pixel that load_halos_t (metrics.hip:51-73) loads in its LAST, partial round:
    R * R is no multiple of 256, so only threads with i < R * R take part.  w = 3: R = 34, 1156 = 4 * 256 + 132;
    w = 5: 1296 = 5 * 256 + 16; w = 11: 1764 = 6 * 256 + 228; w = 15: 2116 = 8 * 256 + 68."""
    R, half = MT + window - 1, window // 2
    rounds = (R * R + MTPB - 1) // MTPB
    rest = R * R - (rounds - 1) * MTPB
    assert 0 < rest < MTPB
    i = (rounds - 1) * MTPB + rest // 2
    return i // R - half, i % R - half


def positions_67x45(window):
    """(y, x, why) on the 67 x 45 image: 3 x 2 tiles, the last tile row 3 rows high and the last tile column 13 wide."""
    g = (3, 4) if window >= 5 else (1, 2)
    ly, lx = last_round_pixel(window)
    pos = [
        # zero padding at the four borders: load_halos_t's `y >= 0 && y < H && x >= 0 && x < W` (:61)
        (0, 0, "corner"), (0, 44, "corner"), (66, 0, "corner"),
        # ... and the ragged last tile: `oy < H && ox < W` in the tile kernel's reduction (:235); y0 = 64, x0 = 32
        (66, 44, "corner, ragged tile"),
        # tile seams: y0, x0 (:145) and the halo origin y0 - HALF, x0 - HALF (:151); a probe on one side is output of one
        # tile and halo of its neighbour
        (31, 10, "row seam"), (32, 10, "row seam"), (63, 20, "row seam 2"), (64, 20, "row seam 2"),
        (10, 31, "column seam"), (10, 32, "column seam"),
        (31, 31, "seam crossing"), (31, 32, "seam crossing"), (32, 31, "seam crossing"), (32, 32, "seam crossing"),
        # the horizontal pass takes columns in pairs 2 xg, 2 xg + 1 with the shift pixel at column 2 xg (:157-159, taps
        # k = j - o :175; kcol in the vertical pass :194): the probe IS the shift pixel at 20 and its neighbour at 21
        (10, 20, "pair, even column"), (10, 21, "pair, odd column"),
        # the vertical pass works in groups of GV rows (:139) recentred on the group's second row (:198-199): rows on both
        # sides of a group boundary (groups 0-3 | 4-7 for windows >= 5, 0-1 | 2-3 for window 3), and a probe that IS a
        # group's centre pixel (row 5, or row 3 for window 3)
        (g[0], 7, "vertical group, last row"), (g[1], 7, "vertical group, first row"),
        (5 if window >= 5 else 3, 8, "vertical group, centre row"),
        # the last, partial round of load_halos_t (:51, `i < R * R` :61 and :70)
        (ly, lx, "last load round"),
    ]
    assert len({(y, x) for y, x, _ in pos}) == len(pos)
    return pos


def positions_33x33(window):
    """(y, x, why) on the 33 x 33 image: 2 x 2 tiles whose ragged ones are one row / one column / one pixel (:235)"""
    return [(0, 0, "corner"), (0, 32, "corner, one-column tile"), (32, 0, "corner, one-row tile"),
            (32, 32, "corner, one-pixel tile"), (31, 31, "seam crossing"), (31, 32, "seam crossing"),
            (32, 31, "seam crossing")]


# The background is random, so a planted fault moves S by a random amount and now and then by too little to count.  Each
# case's seed is the first one, counting up from 1, at which every planted fault that applies moves every image of the case
# by ten bars (tests/test_metrics_local_cpu.py asserts it); nothing about the device enters the choice.
SEEDS = {("67x45", 3): 1, ("67x45", 5): 1, ("67x45", 11): 2, ("67x45", 15): 3, ("33x33", 3): 1, ("33x33", 5): 1,
         ("33x33", 11): 1, ("33x33", 15): 1, ("planes", 5): 1, ("planes", 11): 1, ("many", 1): 1, ("many", 2): 1}

SINGLE_SHAPES = {"67x45": ((67, 45), positions_67x45), "33x33": ((33, 33), positions_33x33)}


@functools.lru_cache(maxsize=None)
def single_probe_case(name, window, seed=None):
    """One image per probe position (C = 1): (shape, probes, why, a, b, affected, S) - S the oracle's sum of (1 - map) per
    image.  Computed once and shared, read-only."""
    (H, W), positions = SINGLE_SHAPES[name]
    pos = positions(window)
    shape = (len(pos), 1, H, W)
    probes = [(i, 0, y, x) for i, (y, x, _) in enumerate(pos)]
    return _case(shape, probes, [w for _, _, w in pos], SEEDS[name, window] if seed is None else seed, window)


def _case(shape, probes, why, seed, window):
    a, b, affected = probe_pair(shape, probes, seed, window)
    S = one_minus_sum(mapped(a, "pm1"), mapped(b, "pm1"), window)
    return dict(shape=shape, probes=probes, why=why, a=a, b=b, affected=affected, S=S, window=window, seed=seed)


# every (b, c) plane of a B = 3, C = 4 batch carries its probe somewhere else: a wrong sb / sc base (:147-148) or a partial
# written to another plane's slot (:254) changes some image's S
PLANES_SHAPE = (3, 4, 67, 45)
PLANES_WINDOWS = (5, 11)


@functools.lru_cache(maxsize=None)
def planes_case(window, seed=None):
    B, C, H, W = PLANES_SHAPE
    probes = [(b, c, (11 * (b * C + c) + 3) % H, (7 * (b * C + c) + 2) % W) for b in range(B) for c in range(C)]
    assert len({(y, x) for _, _, y, x in probes}) == B * C
    return _case(PLANES_SHAPE, probes, ["plane"] * len(probes), SEEDS["planes", window] if seed is None else seed, window)


# more partials than image_metrics_final_kernel has threads: its `i += 256` loop (:272) takes a second trip for 4 of them
MANY_C, MANY_HW, MANY_WINDOW = 65, 33, 11


@functools.lru_cache(maxsize=None)
def many_partials_case(B, seed=None):
    shape = (B, MANY_C, MANY_HW, MANY_HW)
    tiles = ((MANY_HW + MT - 1) // MT) ** 2
    assert MANY_C * tiles > MTPB
    # channel 64's partials are 256 .. 259 (the second trip), channel 0's the first four; the last image of a batch is the
    # one whose partials end the workspace
    probes = [(b, c, y, x) for b in range(B) for (c, y, x) in ((64, 32, 32), (64, 5, 9), (0, 16, 16))]
    return _case(shape, probes, ["final loop"] * len(probes), SEEDS["many", B] if seed is None else seed, MANY_WINDOW)


PROBE_CASES = {**{f"{n}_w{w}": (lambda n=n, w=w: single_probe_case(n, w)) for n in SINGLE_SHAPES for w in WINDOWS},
               **{f"planes_w{w}": (lambda w=w: planes_case(w)) for w in PLANES_WINDOWS},
               **{f"many_partials_B{B}": (lambda B=B: many_partials_case(B)) for B in (1, 2)}}


def probe_case(name):
    """a probe case the device runs, by name (built on first use)"""
    return PROBE_CASES[name]()


def probe_cases():
    for name in PROBE_CASES:
        yield name, probe_case(name)


# ------------------------------------------------------------------------------------------------- small images
SMALL_SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 40), (40, 1))
SMALL_WINDOWS = (3, 11, 15)
SMALL_C = (1, 3)


def closed_form_1x1(a01, b01, window):
    """the formula on a 1 x 1 image: only the centre tap g sees a pixel"""
    g = window2d(window)[window // 2, window // 2]
    mu1, mu2 = g * a01, g * b01
    s1, s2, s12 = g * a01 * a01 - mu1 * mu1, g * b01 * b01 - mu2 * mu2, g * a01 * b01 - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def clear_caches():
    for fn in (single_probe_case, planes_case, many_partials_case):
        fn.cache_clear()
