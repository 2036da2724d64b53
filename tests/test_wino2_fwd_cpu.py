"""CPU side of the F(2x2,3x3) two-level forward (ops.set_winograd_mode("bwd_f2")): the ISA of the GEMM it launches, the option
surface, the entry point's argument checks."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmhand_amd", "csrc")


@pytest.fixture(scope="module")
def igemm_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv_igemm.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950",
                           "-Wno-unused-function", "-Wno-inline-asm", "--cuda-device-only", "-S", "-o", str(out),
                           os.path.join(CSRC, "conv_igemm.hip")])
    return out.read_text().splitlines()


@pytest.mark.parametrize("bn", [128, 64])
def test_two_level_gemm_of_the_16_plane_forward_has_no_scratch_in_its_k_loop(bn, igemm_asm):
    """mmh_wino_gemm_levels16 launches wino_gemm_kernel<BN, 2> (the plane count is only the extent of its work list).  The
    gate of tests/test_host_cpu.py for the 64-plane use, restated for both column widths the 16-plane forward reaches
    (N > 64: 128, N = 64: 64): no scratch access in a block of loop depth >= 2 (the k-loop), no more scratch than the 48
    bytes of tile-constant addresses the persistent loop reloads once per tile, and the k-loop holds the MFMAs."""
    lines = igemm_asm
    start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*wino_gemm_kernelILi%dELi2E\w*:" % bn, l)]
    assert len(start) == 1, start
    name = re.match(r"^(_Z\w+):", lines[start[0]]).group(1)
    end = next(i for i in range(start[0], len(lines)) if lines[i].strip() == f".amdhsa_kernel {name}")
    scratch_bytes = next(int(l.split()[-1]) for l in lines[end:end + 60] if ".amdhsa_private_segment_fixed_size" in l)
    depth, by_depth, mfma_by_depth = 0, {}, {}
    for l in lines[start[0] + 1:end]:
        if re.match(r"^\.LBB\d+_\d+:", l):
            m = re.search(r"Depth=(\d+)", l)
            depth = int(m.group(1)) if m else 0
        elif re.match(r"^\s*;\s+(Parent Loop|=>|Child Loop)", l):
            m = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", l)
            if m:
                depth = int(m.group(1))
        elif "scratch_" in l:
            by_depth[depth] = by_depth.get(depth, 0) + 1
        elif "v_mfma" in l:
            mfma_by_depth[depth] = mfma_by_depth.get(depth, 0) + 1
    print(bn, "scratch bytes", scratch_bytes, "scratch by depth", by_depth, "mfma by depth", mfma_by_depth)
    assert mfma_by_depth.get(2, 0) >= 32, mfma_by_depth
    assert not any(d >= 2 for d in by_depth), by_depth
    assert scratch_bytes <= 48, scratch_bytes


def test_option_parsing():
    from mmhand_amd.options import TrainOptions, check_exact_fwd, default_train_opt
    assert TrainOptions().parse([], save=False).fp32_exact_fwd == "direct"
    assert default_train_opt().fp32_exact_fwd == "direct"
    o = TrainOptions().parse(["--fp32_exact_grads", "--fp32_exact_fwd", "wino2"], save=False)
    assert o.fp32_exact_grads and o.fp32_exact_fwd == "wino2"
    with pytest.raises(SystemExit):
        TrainOptions().parse(["--fp32_exact_fwd", "wino2"], save=False)
    with pytest.raises(SystemExit):
        TrainOptions().parse(["--fp32_exact_grads", "--fp32_exact_fwd", "wino4"], save=False)
    with pytest.raises(ValueError, match="fp32_exact_grads"):
        check_exact_fwd(default_train_opt(fp32_exact_fwd="wino2"))
    check_exact_fwd(default_train_opt(fp32_exact_fwd="wino2", fp32_exact_grads=True))


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from mmhand_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(64)
    assert l.mmh_wino_gemm_levels16(None, p, p, 16, 64, 64, 2, None) != 0
    assert l.mmh_wino_gemm_levels16(p, p, p, 16, 48, 64, 2, None) != 0      # K % 32
    assert l.mmh_wino_gemm_levels16(p, p, p, 16, 64, 32, 2, None) != 0      # N < 64
    assert l.mmh_wino_gemm_levels16(p, p, p, 16, 64, 64, 3, None) != 0      # levels
    assert l.mmh_wino_gemm_levels16(p, p, p, 1 << 30, 64, 64, 2, None) != 0  # too large


def test_mode_names_without_a_gpu(monkeypatch):
    from mmhand_amd import lib, ops
    monkeypatch.setattr(lib, "call", lambda *a: 0)
    keep = (ops.USE_WINOGRAD, ops.WINOGRAD_FPROP, ops.WINO2_FWD)
    try:
        ops.set_winograd_mode("bwd_f2")
        assert ops.USE_WINOGRAD and not ops.WINOGRAD_FPROP and ops.WINO2_FWD
        assert ops._wino_tile(2, 16, 16, 256, 256, 3, 1, 1, False) == 0             # the callers of "bwd" see "bwd"
        assert ops._wino_tile(2, 16, 16, 256, 256, 3, 1, 1, False, "dgrad") == 6
        ops.set_winograd_mode("bwd")
        assert not ops.WINO2_FWD and not ops.WINOGRAD_FPROP
        with pytest.raises(ValueError):
            ops.set_winograd_mode("f2")
    finally:
        ops.USE_WINOGRAD, ops.WINOGRAD_FPROP, ops.WINO2_FWD = keep
