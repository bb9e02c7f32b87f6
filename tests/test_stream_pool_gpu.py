"""GPU: the two stream-pool kernels through `wesep_amd.dev` (csrc/stream.hip: `ws_tcn_mid_stream_rows_fwd`,
`ws_ola_stream_rows_fwd`), for the tables of tests/test_stream_pool_host_cpu.py (tc of 0, 1 and Tc, t0 of 0, taps before the
start, a chunk that wraps its ring, slots in non-ascending order, more slots than rows).

Bit for bit (`torch.equal`): every valid row against the existing solo entry point called on that row alone with R = 1,
Tc = tc[i], t0 = t0[i] -- outputs, the ring row and the carry left behind.  That is derivable, not measured: both kernels
inline one frame / row body, launched with the same number of threads.  State rows of slots outside the table come back
untouched (sentinel), frames behind tc[i] are zeros in y2 and est and (0, 1) in st2, NaN behind tc[i] changes no valid bit, a
second launch repeats the bits.
Against the float64 restatement (tests/emu_stream_pool.py): 1e-5 relative L2, the bound tests/test_stream_fused_gpu.py holds
the fused kernel to -- it is the same arithmetic; the measured worst case is printed."""
import pytest
import torch

from tests import emu_stream_pool
from tests.test_stream_pool_host_cpu import EPS, GEOMS, NSLOTS, TC, as_tables, mid_inputs, ola_inputs, tables

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30))


def _mid(dv, A, H, P, dil, tabs, ring, c=None):
    from wesep_amd import dev
    d = ring.device
    y2, st2 = torch.full((A * TC, H), SENTINEL, device=d), torch.full((A * TC, 2), SENTINEL, device=d)
    dev.tcn_mid_stream_rows_fwd(dv["c"] if c is None else c, dv["rb"], dv["a1"], dv["g1"], dv["b1"], dv["wd"], dv["bd"], dv["a2"], A, TC,
                                H, P, dil, EPS, *tabs, ring, y2, st2)
    return y2.view(A, TC, H), st2.view(A, TC, 2)


@pytest.mark.parametrize("with_rb", [True, False])
@pytest.mark.parametrize("P,dil", GEOMS)
@pytest.mark.parametrize("H", [8, 512, 1028])       # 2 quads (less than a wave), two waves, 257 quads (not a multiple of 64)
def test_tcn_mid_rows_against_the_solo_kernel_and_float64(H, P, dil, with_rb):
    from wesep_amd import dev
    d = _cuda()
    worst = 0.0
    for name, (slot, t0, tc) in tables(P, dil).items():
        A = len(slot)
        v32 = mid_inputs(H, P, dil, A, with_rb=with_rb, dtype=torch.float32)
        dv = {k: (x.to(d) if x is not None else None) for k, x in v32.items()}
        tabs = as_tables(slot, t0, tc, d)
        ring0 = dv["ring"].clone()
        for sl in set(range(NSLOTS)) - set(slot):                    # slots outside the table: a sentinel
            ring0[sl] = SENTINEL
        ring = ring0.clone()
        keep = dv["c"].clone()
        y2, st2 = _mid(dv, A, H, P, dil, tabs, ring)
        assert torch.equal(dv["c"], keep)                            # c is read only
        # (a) bit for bit the solo kernel, row by row; zeros and (0, 1) behind tc; untouched state outside the table
        for i in range(A):
            n, sl = tc[i], slot[i]
            assert not y2[i, n:].any() and not st2[i, n:, 0].any() and (st2[i, n:, 1] == 1).all(), (name, i)
            if n == 0:
                assert torch.equal(ring[sl], ring0[sl]), (name, i)
                continue
            r1 = ring0[sl:sl + 1].clone()
            ys, ss = torch.empty(n, H, device=d), torch.empty(n, 2, device=d)
            dev.tcn_mid_stream_fwd(dv["c"].view(A, TC, H)[i, :n].contiguous(), None if dv["rb"] is None else dv["rb"][sl:sl + 1].contiguous(),
                                   dv["a1"], dv["g1"], dv["b1"], dv["wd"], dv["bd"], dv["a2"], 1, n, H, P, dil, EPS, t0[i], r1, ys, ss)
            assert torch.equal(y2[i, :n], ys) and torch.equal(st2[i, :n], ss) and torch.equal(ring[sl], r1[0]), (name, i)
        for sl in set(range(NSLOTS)) - set(slot):
            assert (ring[sl] == SENTINEL).all(), (name, sl)
        # (b) NaN behind tc changes no bit; a second launch repeats the bits
        cn = dv["c"].clone().view(A, TC, H)
        for i in range(A):
            cn[i, tc[i]:] = float("nan")
        ring_b = ring0.clone()
        y2b, st2b = _mid(dv, A, H, P, dil, tabs, ring_b, c=cn.view(A * TC, H))
        assert torch.equal(y2b, y2) and torch.equal(st2b, st2) and torch.equal(ring_b, ring), name
        # (c) the float64 restatement
        v64 = {k: (x.double() if x is not None else None) for k, x in v32.items()}
        ring64 = v64["ring"].clone()
        y64, s64 = torch.zeros(A * TC, H, dtype=torch.float64), torch.zeros(A * TC, 2, dtype=torch.float64)
        emu_stream_pool.tcn_mid_stream_rows_fwd(v64["c"], v64["rb"], v64["a1"], v64["g1"], v64["b1"], v64["wd"], v64["bd"], v64["a2"], A,
                                                TC, H, P, dil, EPS, *as_tables(slot, t0, tc), ring64, y64, s64)
        y64, s64 = y64.view(A, TC, H), s64.view(A, TC, 2)
        rows = [i for i in range(A) if tc[i] > 0]
        normed = lambda y, s: (y.double().cpu() - s[..., 0:1].double().cpu()) * s[..., 1:2].double().cpu()
        errs = [_rel(torch.cat([y2[i, :tc[i]] for i in rows]), torch.cat([y64[i, :tc[i]] for i in rows])),
                _rel(torch.cat([normed(y2[i, :tc[i]], st2[i, :tc[i]]) for i in rows]),
                     torch.cat([normed(y64[i, :tc[i]], s64[i, :tc[i]]) for i in rows])),
                _rel(torch.stack([ring[slot[i]] for i in rows]), torch.stack([ring64[slot[i]] for i in rows]))]
        print(f"tcn_mid_rows H={H} P={P} dil={dil} rb={with_rb} {name}: vs float64 y2 {errs[0]:.3e} normed {errs[1]:.3e} "
              f"ring {errs[2]:.3e}")
        worst = max(worst, *errs)
        assert all(e < 1e-5 for e in errs), (name, errs)
    print(f"tcn_mid_rows H={H} P={P} dil={dil} rb={with_rb}: worst vs float64 {worst:.3e}")


@pytest.mark.parametrize("Lk,hop", [(20, 10), (16, 8), (40, 10)])
def test_ola_rows_against_the_solo_kernel_and_float64(Lk, hop):
    from wesep_amd import dev
    d = _cuda()
    worst = 0.0
    for name, (slot, t0, tc) in tables(3, 1).items():
        A = len(slot)
        v32 = ola_inputs(Lk, hop, A, dtype=torch.float32)
        dv = {k: x.to(d) for k, x in v32.items()}
        tabs = as_tables(slot, t0, tc, d)
        carry0 = dv["carry"].clone()
        for sl in set(range(NSLOTS)) - set(slot):
            carry0[sl] = SENTINEL

        def run(frames):
            carry, est = carry0.clone(), torch.full((A, TC * hop), SENTINEL, device=d)
            dev.ola_stream_rows_fwd(frames, dv["bias"], A, TC, Lk, hop, *tabs, carry, est)
            return carry, est

        carry, est = run(dv["frames"])
        for i in range(A):
            n, sl = tc[i], slot[i]
            assert not est[i, n * hop:].any(), (name, i)
            if n == 0:
                assert torch.equal(carry[sl], carry0[sl]), (name, i)
                continue
            c1, e1 = carry0[sl:sl + 1].clone(), torch.empty(1, n * hop, device=d)
            dev.ola_stream_fwd(dv["frames"].view(A, TC, Lk)[i, :n].contiguous(), dv["bias"], 1, n, Lk, hop, c1, e1)
            assert torch.equal(est[i, :n * hop], e1[0]) and torch.equal(carry[sl], c1[0]), (name, i)
        for sl in set(range(NSLOTS)) - set(slot):
            assert (carry[sl] == SENTINEL).all(), (name, sl)
        fn = dv["frames"].clone().view(A, TC, Lk)
        for i in range(A):
            fn[i, tc[i]:] = float("nan")
        carry_b, est_b = run(fn.view(A * TC, Lk))
        assert torch.equal(carry_b, carry) and torch.equal(est_b, est), name
        v64 = {k: x.double() for k, x in v32.items()}
        c64, e64 = v64["carry"].clone(), torch.zeros(A, TC * hop, dtype=torch.float64)
        emu_stream_pool.ola_stream_rows_fwd(v64["frames"], v64["bias"], A, TC, Lk, hop, *as_tables(slot, t0, tc), c64, e64)
        rows = [i for i in range(A) if tc[i] > 0]
        errs = [_rel(torch.cat([est[i, :tc[i] * hop] for i in rows]), torch.cat([e64[i, :tc[i] * hop] for i in rows])),
                _rel(torch.stack([carry[slot[i]] for i in rows]), torch.stack([c64[slot[i]] for i in rows]))]
        print(f"ola_rows L={Lk} hop={hop} {name}: vs float64 est {errs[0]:.3e} carry {errs[1]:.3e}")
        worst = max(worst, *errs)
        assert all(e < 1e-5 for e in errs), (name, errs)
    print(f"ola_rows L={Lk} hop={hop}: worst vs float64 {worst:.3e}")


def test_table_entries_that_name_no_slot_touch_no_state():
    """An out-of-range slot or a negative t0 skips the row (zeros out, no state access), tc is clamped to [0, Tc]."""
    from wesep_amd import dev
    d = _cuda()
    P, dil, H, A = 3, 4, 8, 4
    dv = {k: (x.to(d) if x is not None else None) for k, x in mid_inputs(H, P, dil, A, dtype=torch.float32).items()}
    slot, t0, tc = [NSLOTS, 1, -1, 2], [0, -1, 3, 5], [TC, TC, TC, TC + 9]
    ring0 = dv["ring"].clone()
    ring = ring0.clone()
    y2, st2 = _mid(dv, A, H, P, dil, as_tables(slot, t0, tc, d), ring)
    assert not y2[:3].any() and not st2[:3, :, 0].any() and (st2[:3, :, 1] == 1).all()
    keep = [sl for sl in range(NSLOTS) if sl != 2]
    assert torch.equal(ring[keep], ring0[keep]) and not torch.equal(ring[2], ring0[2])
    good, _ = _mid(dv, A, H, P, dil, as_tables(slot, t0, [TC] * 4, d), ring0.clone())
    assert torch.equal(y2[3], good[3])                               # tc above Tc is Tc
    v = {k: x.to(d) for k, x in ola_inputs(20, 10, A, dtype=torch.float32).items()}
    carry, est = v["carry"].clone(), torch.full((A, TC * 10), SENTINEL, device=d)
    dev.ola_stream_rows_fwd(v["frames"], v["bias"], A, TC, 20, 10, *as_tables(slot, t0, [TC, TC, TC, -3], d), carry, est)
    assert not est.any() and torch.equal(carry, v["carry"])
    torch.cuda.synchronize()


def test_wrappers_refuse_what_the_kernels_would_refuse():
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    z = lambda *s: torch.zeros(*s, device=d)
    tabs = as_tables([0, 1], [0, 0], [TC, TC], d)
    with pytest.raises(L.WesepHipError, match=r"cap=5 is below \(P - 1\) \* dil \+ Tc = 6"):
        dev.tcn_mid_stream_rows_fwd(z(2 * TC, 8), None, z(1), z(8), z(8), z(8, 3), z(8), z(1), 2, TC, 8, 3, 1, EPS, *tabs, z(3, 5, 8),
                                    z(2 * TC, 8), z(2 * TC, 2))
    with pytest.raises(L.WesepHipError, match="slot: expected a contiguous torch.int32"):
        dev.tcn_mid_stream_rows_fwd(z(2 * TC, 8), None, z(1), z(8), z(8), z(8, 3), z(8), z(1), 2, TC, 8, 3, 1, EPS, tabs[1], tabs[1],
                                    tabs[2], z(3, 6, 8), z(2 * TC, 8), z(2 * TC, 2))
    with pytest.raises(L.WesepHipError, match="tc holds 2 entries, the call needs 3"):
        dev.ola_stream_rows_fwd(z(3 * TC, 20), z(1), 3, TC, 20, 10, *as_tables([0, 1, 2], [0, 0, 0], [1, 1], d), z(3, 10), z(3, TC * 10))
    with pytest.raises(L.WesepHipError, match="L=25 is not a multiple of hop=10"):
        dev.ola_stream_rows_fwd(z(2 * TC, 25), z(1), 2, TC, 25, 10, *tabs, z(3, 15), z(2, TC * 10))
    torch.cuda.synchronize()
