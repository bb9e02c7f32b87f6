"""GPU: the whole-block kernels through `wesep_amd.dev` (csrc/stream_block.hip: `ws_tcn_block_stream_fwd`,
`ws_tcn_block_stream_rows_fwd`).

Bit for bit (`torch.equal`), which is the kernel's contract and not a measurement: `out` and the ring of one chunk with the
whole 14-frame sequence against three chunkings of it (all ones, fours, sevens -- Tc of 1, 4 and 7); R = 3 against three
R = 1 calls; the rows form on the six tables of tests/test_stream_pool_host_cpu.py against the solo form on each valid row,
ring row included; a second launch on the same buffers.  Every output and ring lies between sentinel guards, rings start as
NaN (frames before the start are never read), frames behind tc[i] are zeros, state rows of unnamed or out-of-range slots
are untouched, NaN in x behind tc[i] changes no valid bit.
Against the float64 restatement (tests/emu_stream_block.py): rel L2 <= 1e-5 over the valid frames of `out` and over the ring
rows -- the bound tests/test_stream_fused_gpu.py and tests/test_stream_pool_gpu.py hold this kernel family to.  The same
figure for the three-call chain that exists (`conv_block_stream(fused=True)`: GEMM, fused middle, GEMM) on the same inputs
is printed beside it."""
import pytest
import torch

from tests import emu_stream_block
from tests.test_stream_pool_host_cpu import NSLOTS, TC, as_tables, tables

pytestmark = pytest.mark.gpu
SENTINEL, EPS, T, E, GUARD = -12345.5, 1e-5, 14, 12, 64
SHAPES = [(8, 8), (32, 64), (132, 516), (256, 512)]                 # (B, H)
GEOMS = [(3, 1), (3, 4), (5, 2)]                                    # (P, dil)
CHUNKINGS = {"ones": [1] * 14, "fours": [4, 4, 4, 2], "sevens": [7, 7]}
NAMES = ("W1", "b1", "a1", "gamma1", "beta1", "wd", "bd", "a2", "gamma2", "beta2", "W2", "b2")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _guarded(shape, fill, device):
    """A tensor of `shape` filled with `fill` between two guards of SENTINEL; (view, whole buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=device)
    buf[GUARD:GUARD + n] = fill
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


_CASES = {}


def _case(B, H, P, dil, with_rb):
    """float32 inputs on the host: computed once per case and left unchanged."""
    key = (B, H, P, dil, with_rb)
    if key not in _CASES:
        g = torch.Generator().manual_seed(B * 7 + H * 3 + P * 11 + dil + int(with_rb))
        rn = lambda *s: torch.randn(*s, generator=g)
        w = dict(W1=rn(H, B + E if with_rb else B) / B ** 0.5, b1=None if with_rb else rn(H) * 0.1, a1=torch.tensor([0.2]),
                 gamma1=torch.rand(H, generator=g) + 0.5, beta1=rn(H) * 0.1, wd=rn(H, P) * 0.5, bd=rn(H) * 0.1,
                 a2=torch.tensor([0.35]), gamma2=torch.rand(H, generator=g) + 0.5, beta2=rn(H) * 0.1, W2=rn(B, H) / H ** 0.5,
                 b2=rn(B) * 0.1)
        _CASES[key] = dict(w=w, rb=rn(NSLOTS, H) * 0.5 if with_rb else None, x=rn(3, T, B), xrows=rn(5, TC, B),
                           past=rn(NSLOTS, (P - 1) * dil + TC, H))
    return _CASES[key]


def _to(v, device=None, dtype=None):
    return None if v is None else v.to(device=device, dtype=dtype)


def _solo(wd_, x, rb, R, Tc, B, H, P, dil, t0, ring, out):
    from wesep_amd import dev
    dev.tcn_block_stream_fwd(x, rb, *(wd_[k] for k in NAMES), R, Tc, B, H, P, dil, EPS, t0, ring, out)


def _run_chunks(wd_, x, rb, R, B, H, P, dil, sizes, device):
    """The 14 frames of x [R, T, B] in chunks; (out [R, T, B], frame-indexed ring [R, T, H]) -- guards checked."""
    cap = (P - 1) * dil + max(sizes)
    ring, ring_buf = _guarded((R, cap, H), float("nan"), device)
    outs, t0 = [], 0
    for n in sizes:
        out, out_buf = _guarded((R * n, B), SENTINEL, device)
        xc = x[:, t0:t0 + n].reshape(R * n, B).contiguous()
        keep = xc.clone()
        _solo(wd_, xc, rb, R, n, B, H, P, dil, t0, ring, out)
        assert _guards_intact(out_buf) and _guards_intact(ring_buf) and torch.equal(xc, keep)
        outs.append(out.view(R, n, B).clone())
        t0 += n
    held = min(cap, T)                                               # frames T - held .. T - 1 are in the ring
    frames = torch.arange(T - held, T, device=device)
    by_frame = torch.full((R, T, H), float("nan"), device=device)
    by_frame[:, T - held:] = ring[:, frames % cap]
    return torch.cat(outs, 1), by_frame, held


@pytest.mark.parametrize("with_rb", [True, False], ids=["rb_ldw1_B_plus_E", "b1_ldw1_B"])
@pytest.mark.parametrize("P,dil", GEOMS)
@pytest.mark.parametrize("B,H", SHAPES)
def test_block_is_chunking_and_row_independent_and_close_to_float64(B, H, P, dil, with_rb):
    from wesep_amd import functional_tasnet as FT
    d = _cuda()
    cs = _case(B, H, P, dil, with_rb)
    w = {k: _to(v, d) for k, v in cs["w"].items()}
    x, rb, R = cs["x"].to(d), _to(cs["rb"], d), 3
    rb3 = None if rb is None else rb[:R].contiguous()
    whole, ring_w, _ = _run_chunks(w, x, rb3, R, B, H, P, dil, [T], d)
    assert torch.isfinite(whole).all() and torch.isfinite(ring_w).all()
    # (a) any chunking gives the bits of one chunk: out, and every frame the ring still holds
    for name, sizes in CHUNKINGS.items():
        got, ring_c, held = _run_chunks(w, x, rb3, R, B, H, P, dil, sizes, d)
        assert torch.equal(got, whole), (name, float((got - whole).abs().max()))
        assert torch.equal(ring_c[:, T - held:], ring_w[:, T - held:]), name
    # (b) a second run repeats the bits; R = 3 is three R = 1 calls, whatever the other rows hold
    again, ring_a, _ = _run_chunks(w, x, rb3, R, B, H, P, dil, [T], d)
    assert torch.equal(again, whole) and torch.equal(ring_a, ring_w)
    for r in range(R):
        one, ring_1, _ = _run_chunks(w, x[r:r + 1], None if rb is None else rb[r:r + 1].contiguous(), 1, B, H, P, dil, [7, 7], d)
        assert torch.equal(one[0], whole[r]) and torch.equal(ring_1[0, T - 7:], ring_w[r, T - 7:]), r
    # (c) the float64 restatement, and the existing three-call chain on the same inputs
    w64 = {k: _to(v, dtype=torch.float64) for k, v in cs["w"].items()}
    cap = (P - 1) * dil + T
    ring64, out64 = torch.full((R, cap, H), float("nan"), dtype=torch.float64), torch.empty(R * T, B, dtype=torch.float64)
    emu_stream_block.tcn_block_stream_fwd(cs["x"].double().reshape(R * T, B), _to(None if cs["rb"] is None else cs["rb"][:R],
                                          dtype=torch.float64), *(w64[k] for k in NAMES), R, T, B, H, P, dil, EPS, 0, ring64, out64)
    frames = torch.arange(T) % cap
    e_out, e_ring = _rel(whole.reshape(R * T, B), out64), _rel(ring_w, ring64[:, frames])
    ring_f = torch.full((R, cap, H), float("nan"), device=d)
    chain = FT.conv_block_stream(x.reshape(R * T, B).contiguous(), rb3, (R, T, "cLN", dil, None), ring_f, 0, w["W1"], w["b1"],
                                 w["a1"], w["gamma1"], w["beta1"], w["wd"], w["bd"], w["a2"], w["gamma2"], w["beta2"], w["W2"],
                                 w["b2"], fused=True)
    c_out, c_ring = _rel(chain, out64), _rel(ring_f[:, frames], ring64[:, frames])
    print(f"tcn_block B={B} H={H} P={P} dil={dil} rb={with_rb}: vs float64 out {e_out:.3e} ring {e_ring:.3e}; "
          f"the three-call chain: out {c_out:.3e} ring {c_ring:.3e}")
    assert e_out <= 1e-5 and e_ring <= 1e-5, (e_out, e_ring)


def _rows(wd_, x, rb, A, B, H, P, dil, tabs, ring, device):
    from wesep_amd import dev
    out, out_buf = _guarded((A * TC, B), SENTINEL, device)
    dev.tcn_block_stream_rows_fwd(x, rb, *(wd_[k] for k in NAMES), A, TC, B, H, P, dil, EPS, *tabs, ring, out)
    assert _guards_intact(out_buf)
    return out.view(A, TC, B).clone()


@pytest.mark.parametrize("with_rb", [True, False], ids=["rb_ldw1_B_plus_E", "b1_ldw1_B"])
@pytest.mark.parametrize("P,dil", GEOMS)
@pytest.mark.parametrize("B,H", SHAPES)
def test_rows_form_against_the_solo_form_and_float64(B, H, P, dil, with_rb):
    d = _cuda()
    cs = _case(B, H, P, dil, with_rb)
    w = {k: _to(v, d) for k, v in cs["w"].items()}
    w64 = {k: _to(v, dtype=torch.float64) for k, v in cs["w"].items()}
    rb = _to(cs["rb"], d)
    worst = 0.0
    for name, (slot, t0, tc) in tables(P, dil).items():
        A = len(slot)
        x = cs["xrows"][:A].reshape(A * TC, B).contiguous().to(d)
        tabs = as_tables(slot, t0, tc, d)
        ring0, ring0_buf = _guarded(tuple(cs["past"].shape), 0.0, d)
        ring0.copy_(cs["past"])
        for sl in set(range(NSLOTS)) - set(slot):                    # slots outside the table: a sentinel
            ring0[sl] = SENTINEL
        ring_buf = ring0_buf.clone()
        ring = ring_buf[GUARD:-GUARD].view_as(ring0)
        keep = x.clone()
        out = _rows(w, x, rb, A, B, H, P, dil, tabs, ring, d)
        assert torch.equal(x, keep) and _guards_intact(ring_buf)
        # (a) bit for bit the solo form, row by row; zeros behind tc; untouched state outside the table
        for i in range(A):
            n, sl = tc[i], slot[i]
            assert not out[i, n:].any(), (name, i)
            if n == 0:
                assert torch.equal(ring[sl], ring0[sl]), (name, i)
                continue
            r1, o1 = ring0[sl:sl + 1].clone(), torch.empty(n, B, device=d)
            _solo(w, x.view(A, TC, B)[i, :n].contiguous(), None if rb is None else rb[sl:sl + 1].contiguous(), 1, n, B, H, P, dil,
                  t0[i], r1, o1)
            assert torch.equal(out[i, :n], o1) and torch.equal(ring[sl], r1[0]), (name, i)
        for sl in set(range(NSLOTS)) - set(slot):
            assert (ring[sl] == SENTINEL).all(), (name, sl)
        # (b) NaN in x behind tc changes no bit; this second launch repeats the bits
        xn = x.clone().view(A, TC, B)
        for i in range(A):
            xn[i, tc[i]:] = float("nan")
        ring_b = ring0.clone()
        out_b = _rows(w, xn.view(A * TC, B), rb, A, B, H, P, dil, tabs, ring_b, d)
        assert torch.equal(out_b, out) and torch.equal(ring_b, ring), name
        # (c) the float64 restatement
        ring64, out64 = cs["past"].double().clone(), torch.zeros(A * TC, B, dtype=torch.float64)
        emu_stream_block.tcn_block_stream_rows_fwd(cs["xrows"][:A].reshape(A * TC, B).double(), _to(cs["rb"], dtype=torch.float64),
                                                   *(w64[k] for k in NAMES), A, TC, B, H, P, dil, EPS, *as_tables(slot, t0, tc),
                                                   ring64, out64)
        out64 = out64.view(A, TC, B)
        rows = [i for i in range(A) if tc[i] > 0]
        errs = [_rel(torch.cat([out[i, :tc[i]] for i in rows]), torch.cat([out64[i, :tc[i]] for i in rows])),
                _rel(torch.stack([ring[slot[i]] for i in rows]), torch.stack([ring64[slot[i]] for i in rows]))]
        worst = max(worst, *errs)
        assert all(e <= 1e-5 for e in errs), (name, errs)
    print(f"tcn_block_rows B={B} H={H} P={P} dil={dil} rb={with_rb}: worst vs float64 {worst:.3e}")


def test_table_entries_that_name_no_slot_touch_no_state():
    d = _cuda()
    B, H, P, dil, A = 32, 64, 3, 4, 4
    cs = _case(B, H, P, dil, True)
    w, rb = {k: _to(v, d) for k, v in cs["w"].items()}, cs["rb"].to(d)
    x = cs["xrows"][:A].reshape(A * TC, B).contiguous().to(d)
    slot, t0, tc = [NSLOTS, 1, -1, 2], [0, -1, 3, 5], [TC, TC, TC, TC + 9]
    ring0 = cs["past"].to(d)
    ring = ring0.clone()
    out = _rows(w, x, rb, A, B, H, P, dil, as_tables(slot, t0, tc, d), ring, d)
    assert not out[:3].any()
    keep = [sl for sl in range(NSLOTS) if sl != 2]
    assert torch.equal(ring[keep], ring0[keep]) and not torch.equal(ring[2], ring0[2])
    good = _rows(w, x, rb, A, B, H, P, dil, as_tables(slot, t0, [TC] * 4, d), ring0.clone(), d)
    assert torch.equal(out[3], good[3]) and torch.isfinite(out[3]).all()          # tc above Tc is Tc
    torch.cuda.synchronize()


def test_wrappers_refuse_what_the_kernels_would_refuse():
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    z = lambda *s: torch.zeros(*s, device=d)
    args = lambda B=8, H=8, P=3: (z(H, B), z(H), z(1), z(H), z(H), z(H, P), z(H), z(1), z(H), z(H), z(B, H), z(B))
    with pytest.raises(L.WesepHipError, match=r"cap=5 is below \(P - 1\) \* dil \+ Tc = 6"):
        dev.tcn_block_stream_fwd(z(8, 8), None, *args(), 2, 4, 8, 8, 3, 1, EPS, 0, z(2, 5, 8), z(8, 8))
    with pytest.raises(L.WesepHipError, match="exactly one of rb"):
        dev.tcn_block_stream_fwd(z(8, 8), z(2, 8), *args(), 2, 4, 8, 8, 3, 1, EPS, 0, z(2, 6, 8), z(8, 8))
    x = z(8, 8)
    with pytest.raises(L.WesepHipError, match="out overlaps x"):
        dev.tcn_block_stream_fwd(x, None, *args(), 2, 4, 8, 8, 3, 1, EPS, 0, z(2, 6, 8), x)
    with pytest.raises(L.WesepHipError, match="H=772 above 768"):
        dev.tcn_block_stream_fwd(z(8, 8), None, *args(H=772), 2, 4, 8, 772, 3, 1, EPS, 0, z(2, 6, 772), z(8, 8))
    tabs = as_tables([0, 1], [0, 0], [4, 4], d)
    with pytest.raises(L.WesepHipError, match="slot: expected a contiguous torch.int32"):
        dev.tcn_block_stream_rows_fwd(z(8, 8), None, *args(), 2, 4, 8, 8, 3, 1, EPS, tabs[1], tabs[1], tabs[2], z(3, 6, 8), z(8, 8))
    torch.cuda.synchronize()
