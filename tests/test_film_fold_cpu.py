"""Host side of the folded speaker-fusion affine (functional.film_fold, dev.Film): the arithmetic the kernels share, restated,
and the argument contracts of the five *_film entry points through the real library (tests/abi_dryrun.py)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

N = 128
SHAPES = [(2, 32, 9), (3, 4, 5)]


def film_ref(z, a, b, a0):
    """csrc/common.h ws_film in torch: fma(z, a0 + a, b) -- the fp32 sum a0 + a, then product and addend rounded ONCE (the
    product of two fp32 numbers is exact in fp64)."""
    return (z.double() * (a0 + a).float().double() + b.double()).float()


def test_film_restated_is_a_correctly_rounded_fma():
    g = torch.Generator().manual_seed(5)
    z, a, b = (torch.randn(3000, generator=g) * s for s in (1.0, 0.5, 0.5))
    b[:1000] = -(z[:1000] * (1.0 + a[:1000]))              # heavy cancellation: where a second rounding of the product would show
    got = film_ref(z, a, b, 1.0).numpy()
    s = (1.0 + a).float().numpy()
    zz, bb = z.numpy(), b.numpy()
    two_roundings = 0
    for i in range(z.numel()):
        exact = Fraction(float(zz[i])) * Fraction(float(s[i])) + Fraction(float(bb[i]))
        c = got[i]
        err = abs(exact - Fraction(float(c)))
        for nb in (np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))):
            assert err <= abs(exact - Fraction(float(nb))), i      # no fp32 number is nearer to the exact value
        two_roundings += int(np.float32(np.float32(zz[i] * s[i]) + bb[i]) != c)
    assert two_roundings > 0                                        # the sample does tell an fma from multiply-then-add


@pytest.mark.skipif(torch.cuda.is_available(), reason="the dry run is for machines without a GPU")
def test_film_fold_is_off_without_a_device(monkeypatch):
    from tests import abi_dryrun
    import wesep_amd.functional as F_
    z = torch.zeros(2, 4, 40, N)
    assert not F_.film_fold(z)
    abi_dryrun.install(monkeypatch)                                  # CPU tensors that claim to be on the device: still off
    assert not torch.cuda.is_available() and not F_.film_fold(z)


@pytest.mark.parametrize("mode", ["FiLM", "multiply", "additive"])
@pytest.mark.parametrize("dims", SHAPES)
def test_film_wrappers_pass_every_contract(dims, mode, monkeypatch):
    """The five wrappers with film=, called directly with the dry-run harness installed: no WS_REQUIRE refuses them."""
    from tests import abi_dryrun
    from wesep_amd import dev
    from wesep_amd.functional import _view_maps
    if torch.cuda.is_available():
        pytest.skip("the dry run is for machines without a GPU")
    calls = abi_dryrun.install(monkeypatch)
    R, K, Tf = dims
    P = R * K * Tf
    geo, smap, seq, _ = _view_maps("time", R, K, Tf, N)
    z = torch.zeros(R, K, Tf, N)
    a = torch.zeros(R, N) if mode != "additive" else None
    b = torch.zeros(R, N) if mode != "multiply" else None
    film = dev.Film(a, b, 0.0 if mode == "multiply" else 1.0, K * Tf)
    ng, nb = geo.ngroups, dev.bl_num_blocks(seq)
    stats, ab, gamma, beta = torch.zeros(ng, 2), torch.zeros(ng, 2), torch.ones(N), torch.zeros(N)
    words = lambda n: torch.zeros(n, dtype=torch.int32)
    dev.group_stats(z, geo, stats, film=film)
    dev.gemm_p2b(A=z.view(P, N), lda=N, sm=seq, Wpack=None, N=0, C_out=None, A_bl=torch.zeros(nb, 32 * N),
                 A_bl16=torch.zeros(dev.blh_floats(nb, N)), stats=stats, gamma=gamma, beta=beta, stat_map=smap, film=film)
    dev.gemm_p2b(A=z.view(P, N), lda=N, sm=seq, Wpack=torch.zeros(1024 * N), N=1024, C_out=torch.zeros(nb, 32 * 1024),
                 stats=stats, gamma=gamma, beta=beta, stat_map=smap, film=film)
    for a_fmt in (0, 4):
        dev.gemm_b2p(A=torch.zeros(nb, 32 * 512), K=512, sm=seq, Wpack=torch.zeros(N * 512), C_out=torch.zeros(P, N), ldc=N,
                     bias=torch.zeros(N), R=z.view(P, N), a_fmt=a_fmt, film=film)
    dxn = torch.zeros(P, N)
    dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma=gamma, film=film)
    tg = dev.tree_groups(ng)
    dev.gn_bwd_apply_pg(z, dxn, stats, ab, geo, torch.zeros_like(z), gamma, torch.zeros(ng + tg, 2, N), torch.zeros(2, N),
                        words(1 + tg), res=torch.zeros_like(z), film=film, fslab=torch.zeros(ng, 2, N),
                        da=torch.zeros(R, N) if a is not None else None, db=torch.zeros(R, N) if b is not None else None,
                        fcounter=words(R))
    assert [w for w, _, _ in calls] == ["ws_group_stats_film", "ws_gemm_p2b_film", "ws_gemm_p2b_film", "ws_gemm_b2p_film",
                                        "ws_gemm_b2p_film", "ws_gn_bwd_reduce_film", "ws_gn_bwd_apply_pg_film"]
    abi_dryrun.assert_contracts_hold(calls, at_least=7)


def test_film_entry_points_refuse_what_they_cannot_fold(monkeypatch):
    """The band view's groups (one per frame, rows Tf * N floats apart) do not tile a row of a / b for the apply pass, and the
    d(xn) formats of ws_gemm_b2p have no residual to fold into: WS_ERR_INVALID, not a launch."""
    from tests import abi_dryrun
    from wesep_amd import dev
    from wesep_amd.functional import _view_maps
    if torch.cuda.is_available():
        pytest.skip("the dry run is for machines without a GPU")
    calls = abi_dryrun.install(monkeypatch)
    R, K, Tf = 2, 4, 6
    P = R * K * Tf
    geo, smap, seq, _ = _view_maps("band", R, K, Tf, N)
    z = torch.zeros(R, K, Tf, N)
    film = dev.Film(torch.zeros(R, N), torch.zeros(R, N), 1.0, K * Tf)
    ng, tg = geo.ngroups, dev.tree_groups(geo.ngroups)
    dev.gn_bwd_apply_pg(z, torch.zeros(P, N), torch.zeros(ng, 2), torch.zeros(ng, 2), geo, torch.zeros_like(z), torch.ones(N),
                        torch.zeros(ng + tg, 2, N), torch.zeros(2, N), torch.zeros(1 + tg, dtype=torch.int32), film=film,
                        fslab=torch.zeros(ng, 2, N), da=torch.zeros(R, N), db=torch.zeros(R, N),
                        fcounter=torch.zeros(ng, dtype=torch.int32))
    nb = dev.bl_num_blocks(seq)
    dev.gemm_b2p(A=torch.zeros(dev.blh_floats(nb, 2048)), K=2048, sm=seq, Wpack=torch.zeros(N * 2048), C_out=torch.zeros(P, N),
                 ldc=N, a_fmt=1, film=film)
    assert [(w, rc) for w, rc, _ in calls] == [("ws_gn_bwd_apply_pg_film", -1), ("ws_gemm_b2p_film", -1)]
