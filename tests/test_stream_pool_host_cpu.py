"""CPU: the two stream-pool kernels (`ws_tcn_mid_stream_rows_fwd`, `ws_ola_stream_rows_fwd`, csrc/stream.hip) without a GPU --
the float64 restatement of tests/emu_stream_pool.py against the existing solo emulations run row by row, for tables that cover
tc of 0, 1 and Tc, t0 of 0, a t0 with taps before the start, a t0 in the middle of a ring wrap, slots in non-ascending order
and more slots than rows; the symbols in the header, the binding and the built library with both ABI numbers unchanged; and
every argument refusal of the two entry points against the real library.  Every test but the emulation's own fails on a tree
without the feature (no symbol)."""
import ctypes
import os
import re

import pytest
import torch

from tests import emu_stream, emu_stream_fused, emu_stream_pool
from wesep_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TC, NSLOTS, EPS = 4, 6, 1e-5
GEOMS = [(3, 1), (3, 4)]                                            # (P, dil)


def cap_of(P, dil, extra=0):
    return (P - 1) * dil + TC + extra


def tables(P, dil, extra=0):
    """name -> (slot, t0, tc): A rows of a [A][TC] rectangle over NSLOTS state slots (more slots than rows, every time)."""
    cap = cap_of(P, dil, extra)
    wrap = 3 * cap - 2                                              # frames cap-2 .. cap+1 of the ring: the chunk wraps
    out = {
        # tc of 0, 1 and Tc; t0 = 0; a t0 with some taps before the start; a t0 in the middle of a wrap; slots descending
        "edges": ([5, 3, 2, 0], [0, dil, wrap, 7 * cap + 1], [1, TC, TC, 0]),
        "one_row": ([4], [wrap], [TC]),
        "all_idle_but_one": ([1, 0, 5], [11, 0, 2], [0, 3, 0]),
        "start_mid_tap": ([2, 5, 1], [1, 2 * dil - 1, 0], [2, TC, 1]),
    }
    g = torch.Generator().manual_seed(100 * P + dil + extra)
    for k in range(2):
        A = 5
        out[f"random{k}"] = (torch.randperm(NSLOTS, generator=g)[:A].tolist(),
                             torch.randint(0, 5 * cap, (A,), generator=g).tolist(),
                             torch.randint(0, TC + 1, (A,), generator=g).tolist())
    return out


def as_tables(slot, t0, tc, device="cpu"):
    return (torch.tensor(slot, dtype=torch.int32, device=device), torch.tensor(t0, dtype=torch.int64, device=device),
            torch.tensor(tc, dtype=torch.int32, device=device))


def mid_inputs(H, P, dil, A, extra=0, with_rb=True, dtype=torch.float64):
    g = torch.Generator().manual_seed(1000 * P + 10 * dil + H + A)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(c=r(A * TC, H) * 1.5 + 0.3, rb=r(NSLOTS, H) * 0.7 if with_rb else None, a1=torch.tensor([0.2]),
             g1=torch.rand(H, generator=g) + 0.5, b1=r(H) * 0.1, wd=r(H, P) * 0.5, bd=r(H) * 0.1, a2=torch.tensor([0.35]),
             ring=r(NSLOTS, cap_of(P, dil, extra), H))               # the past of every slot: random, finite
    return {k: (v.to(dtype) if v is not None else None) for k, v in d.items()}


def ola_inputs(Lk, hop, A, dtype=torch.float64):
    g = torch.Generator().manual_seed(Lk * 31 + hop + A)
    d = dict(frames=torch.randn(A * TC, Lk, generator=g), bias=torch.randn(1, generator=g),
             carry=torch.randn(NSLOTS, Lk - hop, generator=g))
    return {k: v.to(dtype) for k, v in d.items()}


def _close(a, b, tol=1e-11):
    return torch.allclose(a, b, rtol=tol, atol=tol)


@pytest.mark.parametrize("with_rb", [True, False])
@pytest.mark.parametrize("P,dil", GEOMS)
def test_mid_restatement_is_the_solo_emulation_row_by_row(P, dil, with_rb):
    H = 8
    for name, (slot, t0, tc) in tables(P, dil).items():
        A = len(slot)
        v = mid_inputs(H, P, dil, A, with_rb=with_rb)
        ring0, ring = v["ring"].clone(), v["ring"].clone()
        y2, st2 = torch.full((A * TC, H), 7.0, dtype=torch.float64), torch.full((A * TC, 2), 7.0, dtype=torch.float64)
        emu_stream_pool.tcn_mid_stream_rows_fwd(v["c"], v["rb"], v["a1"], v["g1"], v["b1"], v["wd"], v["bd"], v["a2"], A, TC, H, P,
                                                dil, EPS, *as_tables(slot, t0, tc), ring, y2, st2)
        y2, st2 = y2.view(A, TC, H), st2.view(A, TC, 2)
        for i in range(A):
            n, sl = tc[i], slot[i]
            assert not y2[i, n:].any() and not st2[i, n:, 0].any() and (st2[i, n:, 1] == 1).all(), (name, i)
            if n == 0:
                assert torch.equal(ring[sl], ring0[sl]), (name, i)
                continue
            r1 = ring0[sl:sl + 1].clone()
            ys, ss = torch.empty(n, H, dtype=torch.float64), torch.empty(n, 2, dtype=torch.float64)
            emu_stream_fused.tcn_mid_stream_fwd(v["c"].view(A, TC, H)[i, :n].contiguous(), None if v["rb"] is None else v["rb"][sl:sl + 1],
                                                v["a1"], v["g1"], v["b1"], v["wd"], v["bd"], v["a2"], 1, n, H, P, dil, EPS, t0[i], r1,
                                                ys, ss)
            assert _close(y2[i, :n], ys) and _close(st2[i, :n], ss) and _close(ring[sl], r1[0]), (name, i)
        for sl in set(range(NSLOTS)) - set(slot):                    # slots outside the table: untouched
            assert torch.equal(ring[sl], ring0[sl]), (name, sl)


def test_mid_restatement_reads_no_ring_before_the_start_and_no_c_behind_tc():
    P, dil, H = 3, 4, 8
    slot, t0, tc = [2, 0], [0, 3], [TC, 2]
    v = mid_inputs(H, P, dil, 2)
    ref_ring = v["ring"].clone()
    outs = []
    for poison in (False, True):
        ring, c = ref_ring.clone(), v["c"].clone()
        if poison:
            ring[2] = float("nan")                                   # t0 = 0: nothing of slot 2's ring is read
            c.view(2, TC, H)[1, 2:] = float("nan")                   # behind tc
        y2, st2 = torch.empty(2 * TC, H, dtype=torch.float64), torch.empty(2 * TC, 2, dtype=torch.float64)
        emu_stream_pool.tcn_mid_stream_rows_fwd(c, v["rb"], v["a1"], v["g1"], v["b1"], v["wd"], v["bd"], v["a2"], 2, TC, H, P, dil,
                                                EPS, *as_tables(slot, t0, tc), ring, y2, st2)
        outs.append((y2, st2))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(outs[1][0]).all()


@pytest.mark.parametrize("Lk,hop", [(20, 10), (16, 8), (40, 10)])
def test_ola_restatement_is_the_solo_emulation_row_by_row(Lk, hop):
    for name, (slot, t0, tc) in tables(3, 1).items():
        A = len(slot)
        v = ola_inputs(Lk, hop, A)
        carry0, carry = v["carry"].clone(), v["carry"].clone()
        est = torch.full((A, TC * hop), 7.0, dtype=torch.float64)
        emu_stream_pool.ola_stream_rows_fwd(v["frames"], v["bias"], A, TC, Lk, hop, *as_tables(slot, t0, tc), carry, est)
        for i in range(A):
            n, sl = tc[i], slot[i]
            assert not est[i, n * hop:].any(), (name, i)
            if n == 0:
                assert torch.equal(carry[sl], carry0[sl])
                continue
            c1, e1 = carry0[sl:sl + 1].clone(), torch.empty(1, n * hop, dtype=torch.float64)
            emu_stream.ola_stream_fwd(v["frames"].view(A, TC, Lk)[i, :n].contiguous(), v["bias"], 1, n, Lk, hop, c1, e1)
            # (the solo emulation accumulates in float32 whatever it is given: a few float32 roundings of sums of size ~3)
            assert _close(est[i, :n * hop], e1[0], 1e-5) and _close(carry[sl], c1[0], 1e-5), (name, i)
        for sl in set(range(NSLOTS)) - set(slot):
            assert torch.equal(carry[sl], carry0[sl])


def test_restatement_skips_entries_that_name_no_slot_and_clamps_tc():
    P, dil, H = 3, 1, 8
    v = mid_inputs(H, P, dil, 3)
    ring = v["ring"].clone()
    y2, st2 = torch.full((3 * TC, H), 7.0, dtype=torch.float64), torch.full((3 * TC, 2), 7.0, dtype=torch.float64)
    emu_stream_pool.tcn_mid_stream_rows_fwd(v["c"], v["rb"], v["a1"], v["g1"], v["b1"], v["wd"], v["bd"], v["a2"], 3, TC, H, P, dil,
                                            EPS, *as_tables([NSLOTS, 1, 2], [0, -1, 5], [TC, TC, TC + 9]), ring, y2, st2)
    assert not y2.view(3, TC, H)[:2].any() and torch.equal(ring[:2], v["ring"][:2]) and y2.view(3, TC, H)[2].all()
    assert not torch.equal(ring[2], v["ring"][2])


# ---- the real library -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    for name, nargs, wrapper in (("ws_tcn_mid_stream_rows_fwd", 23, "tcn_mid_stream_rows_fwd"),
                                 ("ws_ola_stream_rows_fwd", 13, "ola_stream_rows_fwd")):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == nargs
        assert name in L.EXPORTED_SYMBOLS and getattr(L.lib(), name) is not None
        from wesep_amd import dev
        assert callable(getattr(dev, wrapper))
    assert L.lib().ws_abi_version() == 20 == L.ABI_VERSION          # new symbols only
    assert re.search(r"^#define WS_ABI_VERSION 20\b", header, flags=re.M)


def test_engine_symbols_are_declared_bound_and_exported():
    from wesep_amd import engine as E
    header = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in ("ws_engine_pool_open", "ws_engine_pool_attach", "ws_engine_pool_push", "ws_engine_pool_flush",
                 "ws_engine_pool_detach", "ws_engine_pool_close"):
        assert re.search(r"^(int|void)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in E.SYMBOLS and hasattr(lib, name) and getattr(E.lib(), name).argtypes is not None
    assert re.search(r"^#define WS_ENGINE_ABI_VERSION 2\b", header, flags=re.M)
    assert E.lib().ws_engine_abi_version() == 2 == E.ENGINE_ABI_VERSION
    assert re.search(r"#define WS_POOL_GROUP_LAUNCHES\(R, X\) \(3 \* \(R\) \* \(X\) \+ 9\)", header)
    assert E.pool_group_launches(2, 3) == 27
    assert callable(E.Engine.stream_pool) and all(hasattr(E.StreamPool, f) for f in ("attach", "push", "flush", "detach", "close"))


def _bufs(n):
    return [ctypes.cast((ctypes.c_float * 8192)(), ctypes.c_void_p) for _ in range(n)]


def test_mid_rows_refuses_bad_arguments_before_any_launch():
    lib = L.lib()
    c, rb, a1, g1, b1, wd, bd, a2, ring, y2, st2, slot, t0, tc = _bufs(14)
    err = lambda: lib.ws_last_error().decode()
    eps = ctypes.c_float(1e-5)

    def call(c=c, rb=rb, a1=a1, g1=g1, b1=b1, wd=wd, bd=bd, a2=a2, A=2, Tc=5, H=8, P=3, dil=4, nslots=3, slot=slot, t0=t0, tc=tc,
             cap=13, ring=ring, y2=y2, st2=st2):
        return lib.ws_tcn_mid_stream_rows_fwd(c, rb, a1, g1, b1, wd, bd, a2, A, Tc, H, P, dil, eps, nslots, slot, t0, tc, cap, ring,
                                              y2, st2, None)

    for name in ("c", "a1", "g1", "b1", "wd", "bd", "a2", "ring", "y2", "st2"):          # every pointer but rb
        assert call(**{name: None}) == -1 and "ws_tcn_mid_stream_rows_fwd: null pointer" in err(), name
    for name in ("slot", "t0", "tc"):
        assert call(**{name: None}) == -1 and "ws_tcn_mid_stream_rows_fwd: a NULL table" in err(), name
    assert call(A=0) == -1 and "bad tables (A=0 rows, nslots=3)" in err()
    assert call(nslots=0) == -1 and "bad tables (A=2 rows, nslots=0)" in err()
    assert call(Tc=0) == -1 and "bad geometry" in err()
    assert call(H=6) == -1 and "H=6 is not a multiple of 4" in err()
    assert call(H=4100) == -1 and "H=4100 above 4096" in err()
    assert call(P=4, cap=17) == -1 and "P=4 (odd P <= 7)" in err()
    assert call(P=9, cap=37) == -1 and "P=9 (odd P <= 7)" in err()
    assert call(dil=0) == -1 and "bad geometry" in err()
    assert call(cap=12) == -1 and "cap=12 is below (P - 1) * dil + Tc = 13" in err()
    assert call(y2=c) == -1 and "y2 overlaps c" in err()
    assert call(A=65536, Tc=32768, cap=32776) == -1 and "A * Tc reaches 2^31" in err()


def test_ola_rows_refuses_bad_arguments_before_any_launch():
    lib = L.lib()
    frames, bias, carry, est, slot, t0, tc = _bufs(7)
    err = lambda: lib.ws_last_error().decode()

    def call(frames=frames, bias=bias, A=2, Tc=5, Lk=20, hop=10, nslots=3, slot=slot, t0=t0, tc=tc, carry=carry, est=est):
        return lib.ws_ola_stream_rows_fwd(frames, bias, A, Tc, Lk, hop, nslots, slot, t0, tc, carry, est, None)

    for name in ("frames", "est"):
        assert call(**{name: None}) == -1 and "ws_ola_stream_rows_fwd: frames or est is NULL" in err(), name
    for name in ("slot", "t0", "tc"):
        assert call(**{name: None}) == -1 and "ws_ola_stream_rows_fwd: a NULL table" in err(), name
    assert call(A=0) == -1 and "bad tables (A=0 rows, nslots=3)" in err()
    assert call(nslots=-1) == -1 and "bad tables" in err()
    assert call(Tc=0) == -1 and "ws_ola_stream_rows_fwd: bad args" in err()
    assert call(hop=0) == -1 and "bad args" in err()
    assert call(Lk=25) == -1 and "L=25 is not a multiple of hop=10" in err()
    assert call(carry=None) == -1 and "carry is NULL (L > hop)" in err()
    assert call(Lk=32768, hop=8192) == -1 and "above 16384" in err()
    assert call(Tc=1 << 27, Lk=16, hop=16) == -1 and "Tc * hop + L reaches 2^31" in err()
