"""The premises of tests/test_norm_exact_gpu.py, checked without a GPU: every dyadic case meets the conditions that make it
exact (tests/_norm_oracle.py: check_any_order, check_forms), the float64 references are what autograd gives for the plain
formula, the plane kernel's geometry per case is the one the case list claims, and the statistics bound holds for a float32
emulation of the kernel's order of operations while staying far below what a dropped row does."""
import pytest
import torch

from tests import _norm_oracle as NO


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cached_cases():
    yield
    NO.clear_caches()


def _id(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("masked,drop_p", [(0, 0.0), (1, 0.5), (1, 0.0)], ids=["unmasked", "keep_p0.5", "keep_p0"])
@pytest.mark.parametrize("shape", NO.TWO_PASS, ids=_id)
def test_two_pass_cases_are_exact(shape, masked, drop_p):
    info = NO.check_dyadic(NO.two_pass_case(shape, masked, drop_p), f"two-pass {shape}")
    assert info.max_s2 <= 9928 * 4 and info.max_dx <= 664 * 4       # small dyadic values, nowhere near 2^24


@pytest.mark.parametrize("masked,drop_p", [(0, 0.0), (1, 0.5)], ids=["unmasked", "keep_p0.5"])
@pytest.mark.parametrize("shape", NO.TWO_PASS_BATCH, ids=_id)
def test_batch_grouped_cases_are_exact(shape, masked, drop_p):
    NO.check_dyadic(NO.two_pass_case(shape, masked, drop_p, batch=True), f"two-pass, one group {shape}")


@pytest.mark.parametrize("relu,drop_p", NO.RC_MODES, ids=["relu_p0.5", "relu_p0", "plain"])
@pytest.mark.parametrize("shape", NO.RC_SHAPES, ids=_id)
def test_rc_cases_are_exact(shape, relu, drop_p):
    P = NO.rc_case(shape, relu, drop_p)
    NO.check_any_order(P.dz, P.x, P.mean, P.invstd, f"rc {shape}")
    NO.check_forms(P.dz, P.s1, P.s2, P.x, P.mean, P.invstd, P.gamma, P.count, P.dx, f"rc {shape}")
    NO.check_forms(P.dz, P.s1, P.s2, P.x, P.mean, P.invstd, None, P.count, P.dx_plain, f"rc {shape} gamma NULL")
    if relu:
        kept = float(P.keep.double().mean())
        assert 0.1 < kept < 0.9, kept       # the recomputed ReLU really decides


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape", sorted({c[0] for c in NO.PLANE}), ids=_id)
def test_plane_cases_are_exact(shape, masked):
    NO.check_dyadic(NO.plane_case(shape, masked), f"plane {shape}")


@pytest.mark.parametrize("case", NO.PLANE, ids=lambda c: _id(c[0]) + "-" + c[1])
def test_plane_cases_select_the_geometry_they_claim(case):
    """plane_lpr_log2 transcribed: the lanes per row, and whether some slot lies past the plane (the kernel's `tail`)"""
    (B, H, W, C), g, l, tail = case
    rows = H * W
    assert NO.plane_lpr_log2(rows, C, g) == l
    assert NO.plane_has_tail(rows, C, g) == tail
    nslots, NR = NO.FT >> l, NO.plane_nr(g)
    assert rows <= nslots * NR                                      # the plane fits
    assert tail == (nslots * NR != rows)
    assert NO.plane_lpr_log2(NO.FT * NR + 1, C, g) == -1            # and one row past the cap does not


def test_plane_cases_cover_every_geometry():
    assert {c[2] for c in NO.PLANE} == {0, 1, 2, 3}
    assert {(c[1], c[3]) for c in NO.PLANE} == {("g16", True), ("g16", False), ("f32", True), ("f32", False)}


@pytest.mark.parametrize("shape", NO.PROD, ids=_id)
def test_production_count_cases_keep_exact_sums(shape):
    """count = rows: dx is not exact, the sums still are"""
    for masked in (False, True):
        P = NO.prod_case(shape, masked)
        assert P.count == shape[1] * shape[2] and P.count != NO.next_pow2(P.count)
        NO.check_any_order(P.dz, P.x, P.mean, P.invstd, f"production count {shape}")
        want, allow = NO.prod_bound(P, P.gamma, "f32")
        assert float((want - P.dx).abs().max()) <= 1e-12 * float(P.dx.abs().max()) and float(allow.min()) >= 0


@pytest.mark.parametrize("chunks", NO.SUMS_FINAL_CHUNKS)
def test_sums_final_cases_are_exact(chunks):
    P = NO.sums_final_case(chunks)
    assert float(P.part.abs().sum(1).max()) < 2 ** 24 and torch.equal(P.part, P.part.round())


@pytest.mark.parametrize("shape", NO.GATE, ids=_id)
def test_gate_cases_are_exact(shape):
    P = NO.gate_case(shape)
    for t in (P.s1, P.out):
        assert NO.is_f32(t)
    assert torch.equal(P.s1 * 2, (P.s1 * 2).round()) and float(P.s1.abs().max()) <= 18
    for absent in NO.GATE_ABSENT:
        Rf = NO.gate_bwd_ref(P, *absent)
        assert torch.equal(Rf.g_x1 / 4, (Rf.g_x1 / 4).round()) and float(Rf.g_x1.abs().max()) <= 36
        for t in (Rf.g_x1, Rf.g_s1, Rf.g_s2, Rf.g_s3, Rf.g_x1 * P.s1, Rf.g_s1 * Rf.xhat):
            assert NO.is_f32(t)
        assert float(Rf.g_s2.abs().max()) <= 93 and float(Rf.g_s3.abs().max()) <= 93
        # the sums in any order: integers times invstd
        assert float(((Rf.g_s1 * Rf.xhat).abs().sum(1) / NO.MIN_INVSTD).max()) < 2 ** 24


def test_dx_rounding_is_exercised():
    """a good share of the exact dx values are NOT representable in bf16: the single rounding is really tested"""
    P = NO.two_pass_case((2, 37, 29, 64), 1, 0.5)
    share = float((NO.stored(P.dx, "bf16") == P.dx).double().mean())
    assert 0.05 <= share <= 0.7, share
    assert torch.equal(NO.stored(P.dx, "f32"), P.dx)


# ------------------------------------------------------------------------------------------------ the references
def test_references_match_autograd_of_the_plain_formula():
    """norm_bwd_ref against autograd of float64 ((x - mean(x)) * invstd(x) * gamma) with the statistics of x itself and
    count = rows (the closed form, not F.instance_norm), under a keep mask and dsc = 2"""
    gen = torch.Generator().manual_seed(5)
    G, rows, C = 2, 37, 8
    x = torch.randn(G, rows, C, generator=gen, dtype=torch.float64).requires_grad_(True)
    gamma = torch.randn(C, generator=gen, dtype=torch.float64)
    g = torch.randn(G, rows, C, generator=gen, dtype=torch.float64)
    keep = torch.rand(G, rows, C, generator=gen) < 0.6
    mean = x.mean(1, keepdim=True)
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    y = (x - mean) * invstd * gamma
    y.backward(g * keep * 2.0)
    _, s1, s2, dx = NO.norm_bwd_ref(g, keep, 2.0, x.detach(), mean.detach()[:, 0], invstd.detach()[:, 0], gamma, float(rows))
    # autograd differentiates THROUGH the statistics; with mean / invstd the statistics of x and eps inside invstd the
    # closed form is the same function
    assert float((dx - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_gate_reference_matches_autograd():
    """gate_bwd_ref at s2 = s3 = 0 against autograd of out = x1 + s1 sigmoid(s2) sigmoid(s3) and the two concats"""
    gen = torch.Generator().manual_seed(6)
    rows, C = 11, 8
    x1, y2 = (torch.randn(1, rows, C, generator=gen, dtype=torch.float64) for _ in range(2))
    scale, shift = torch.randn(1, C, generator=gen, dtype=torch.float64), torch.randn(1, C, generator=gen, dtype=torch.float64)
    s1 = (y2 * scale[:, None] + shift[:, None]).requires_grad_(True)
    s2 = torch.zeros(1, rows, C, dtype=torch.float64, requires_grad=True)
    s3 = torch.zeros(1, rows, C, dtype=torch.float64, requires_grad=True)
    x1 = x1.requires_grad_(True)
    out = x1 + s1 * torch.sigmoid(s2) * torch.sigmoid(s3)
    x2n, x3n = torch.cat([s3, out], -1), torch.cat([s2, out], -1)
    g_out, g2, g3 = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((1, rows, C), (1, rows, 2 * C), (1, rows, 2 * C)))
    torch.autograd.backward([out, x2n, x3n], [g_out, g2, g3])
    Q = NO.SimpleNamespace(C=C, x1=x1.detach(), y2=y2, s1=s1.detach(), g_out=g_out, g_x2n=g2, g_x3n=g3,
                           mean=torch.zeros(1, C), invstd=torch.ones(1, C))
    Rf = NO.gate_bwd_ref(Q, True, True, True)
    for got, want in ((Rf.g_x1, x1.grad), (Rf.g_s1, s1.grad), (Rf.g_s2, s2.grad), (Rf.g_s3, s3.grad)):
        assert float((got - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ statistics
# (groups, rows, C, second generation): the shapes of the GPU test in the generation(s) they can take, and the strided call
EMULATED = [(2, 1073, 64, True), (2, 1073, 64, False), (1, 6561, 96, False), (3, 36, 24, False), (1, 35, 1024, True),
            (1, 35, 1024, False), (2, 9, 8, True), (2, 9, 8, False), (1, 1073, 64, False)]
# many rows AND many row lanes: 127 and 255 float merges.  The emulation stays inside the bound here too, but a worst-case
# bound that counts one rounding of size u R per merge is no longer below 1/8 of a dropped row's effect (0.024 / 8 at 8192
# rows), so these shapes are not among the GPU cases
EMULATED_ONLY = [(1, 4096, 16, True), (1, 8192, 8, True)]


@pytest.mark.parametrize("case", EMULATED + EMULATED_ONLY, ids=_id)
def test_statistics_bound_holds_for_the_emulated_kernel_and_sees_a_dropped_row(case, capsys):
    """both requirements on the bound of tests/_norm_oracle.py section 4: the float32 emulation of the kernel's order stays
    inside it, and it is at most 1/8 of what dropping either sentinel row does to that channel's mean and M2"""
    groups, rows, C, v2 = case
    P = NO.stats_case(groups, rows, C)
    merges = NO.stats_merges(rows, C, v2)
    mean, m2 = NO.emulate_stats(P.x, groups, rows, C, v2)
    rm, rq = NO.stats_ratio(mean, m2, P, merges)
    with capsys.disabled():
        print(f"\n[stats bound] emulation {case}: |mean - want| / bound = {rm:.3f}, M2 {rq:.3f}")
    assert rm <= NO.STATS_FINDING and rq <= NO.STATS_FINDING, (rm, rq)
    if case in EMULATED_ONLY:
        return
    mb, qb = NO.stats_bound(P.x.double(), merges)
    dm, dq = NO.sentinel_effect(P.x.double())
    assert bool((mb <= dm / 8).all()), (float(mb.max()), float(dm.min()))
    assert bool((qb <= dq / 8).all()), (float(qb.max()), float(dq.min()))


@pytest.mark.parametrize("chunks", NO.MERGE_CHUNKS)
def test_merge_cases_have_the_empty_partials_they_claim(chunks):
    P = NO.merge_case(chunks)
    n = P.part[:, :, 0]
    assert P.count > 0 and bool((n.sum(1) == P.count).all())
    if chunks > 1:
        assert bool((n[:, 0] == 0).all()) and bool((n[:, 2::8] == 0).all())
    assert bool((P.m2 > 0).all())


def test_keep_layouts_agree():
    keep = torch.rand(3, 5, 16, generator=torch.Generator().manual_seed(1)) < 0.5
    kb, db = NO.keep_bytes(keep), NO.drop_bytes(keep)
    for e in range(8):
        # the 16 bits a second-generation lane reads for its 8 channels: low nibbles of two bytes
        two = kb.reshape(3, 5, 2, 2).to(torch.int32)
        word = two[..., 0] | (two[..., 1] << 8)
        assert torch.equal(((word >> (e if e < 4 else e + 4)) & 1).bool(), keep.reshape(3, 5, 2, 8)[..., e])
        assert torch.equal(((db.to(torch.int32) >> e) & 1).bool(), keep.reshape(3, 5, 2, 8)[..., e])


# ------------------------------------------------------------------------------------------------ conv epilogues
@pytest.mark.parametrize("case", NO.NBR, ids=lambda c: _id(c[0]) + ("-reflect" if c[1] else "-zero") + ("-batch" if c[2] else ""))
def test_dgrad_epilogue_cases_are_exact(case):
    """the any-order condition on the ACTUAL dx of the integer problem (the kernel sums it in its own order)"""
    P = NO.nbr_case(case)
    assert torch.equal(P.conv.dx, P.conv.dx.round()) and float(P.conv.dx.abs().max()) <= 256
    NO.check_any_order(P.dz, P.x, P.mean, P.invstd, f"dgrad_nbr {case}")
    assert NO.is_f32(P.s1) and NO.is_f32(P.s2)


@pytest.mark.parametrize("kind", sorted(NO.EPI_STATS))
def test_epilogue_statistics_problems_meet_their_cap(kind):
    P = NO.epi_problem(kind)        # asserts integer-valued and |y| <= 16
    assert float(P.y.abs().max()) <= NO.EPI_CAP and float((P.y != 0).double().mean()) > 0.5
