"""CPU: the whole-block streaming path without a GPU -- the float64 restatement of tests/emu_stream_block.py against the
composition of the restatements that exist (1x1 product, tests/emu_stream_fused.tcn_mid_stream_fwd, 1x1 product with
residual) over EVERY chunking of a 13-frame sequence into chunks of 1 to 5, the rows form's table rules, and the host side
of `ConvTasNetStreamer(block=True)` on the emulation against `fused=True` and the model's whole-utterance forward.  Every
test fails without the feature (no keyword, no `dev` entry point)."""
import pytest
import torch

from tests import emu_stream_block, emu_stream_fused
from tests.test_stream_fused_host_cpu import make_fused_case
from tests.test_stream_tasnet_host_cpu import SMALL, T_TOTAL, chunkings, rel, stream, whole

EPS = 1e-5
T13 = 13


def compositions(total, lo=1, hi=5):
    if total == 0:
        yield []
        return
    for n in range(lo, min(hi, total) + 1):
        for rest in compositions(total - n, lo, hi):
            yield [n] + rest


def params(B, H, P, E, with_rb, R, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    ldw1 = B + E if with_rb else B
    return dict(W1=rn(H, ldw1) / B ** 0.5, b1=None if with_rb else rn(H) * 0.1, rb=rn(R, H) * 0.3 if with_rb else None,
                a1=torch.tensor([0.2], dtype=dtype), gamma1=torch.rand(H, generator=g, dtype=dtype) + 0.5, beta1=rn(H) * 0.1,
                wd=rn(H, P) * 0.5, bd=rn(H) * 0.1, a2=torch.tensor([0.35], dtype=dtype),
                gamma2=torch.rand(H, generator=g, dtype=dtype) + 0.5, beta2=rn(H) * 0.1, W2=rn(B, H) / H ** 0.5, b2=rn(B) * 0.1)


def block_call(w, x, R, Tc, B, H, P, dil, t0, ring, out, rb="own"):
    emu_stream_block.tcn_block_stream_fwd(x, w["rb"] if rb == "own" else rb, w["W1"], w["b1"], w["a1"], w["gamma1"], w["beta1"],
                                          w["wd"], w["bd"], w["a2"], w["gamma2"], w["beta2"], w["W2"], w["b2"], R, Tc, B, H, P,
                                          dil, EPS, t0, ring, out)


def composed_call(w, x, R, Tc, B, H, P, dil, t0, ring, out):
    """The three calls the block replaces, on the existing restatements: product, the fused middle, product + residual."""
    c = x @ w["W1"][:, :B].T + (0.0 if w["rb"] is not None else w["b1"])
    y2, st2 = torch.empty(R * Tc, H, dtype=x.dtype), torch.empty(R * Tc, 2, dtype=x.dtype)
    emu_stream_fused.tcn_mid_stream_fwd(c.contiguous(), w["rb"], w["a1"], w["gamma1"], w["beta1"], w["wd"], w["bd"], w["a2"], R, Tc,
                                        H, P, dil, EPS, t0, ring, y2, st2)
    out[:] = x + w["b2"] + ((y2 - st2[:, 0:1]) * st2[:, 1:2] * w["gamma2"] + w["beta2"]) @ w["W2"].T


@pytest.mark.parametrize("with_rb", [True, False], ids=["rb_ldw1_B_plus_E", "b1_ldw1_B"])
def test_restated_block_is_the_composition_over_every_chunking_of_13_frames(with_rb):
    """P 3, dil 2, cap = 4 + 5 = 9 < 13: chunks wrap the ring; the first chunk has t0 = 0 and taps before the start."""
    R, B, H, P, dil, E = 2, 4, 8, 3, 2, 4
    w = params(B, H, P, E, with_rb, R)
    x = torch.randn(R, T13, B, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    cap = (P - 1) * dil + 5
    steps, tally = {}, {"chunkings": 0, "worst": 0.0}

    def step(t0, Tc, rings):
        """One chunk on both restatements from the given ring contents.  A chunk's result is a function of (t0, Tc, ring
        contents) alone, so a step that many chunkings share is computed once -- every chunking is still walked to its end."""
        key = (t0, Tc, rings[0].numpy().tobytes(), rings[1].numpy().tobytes())
        if key not in steps:
            after = [r.clone() for r in rings]
            xc = x[:, t0:t0 + Tc].reshape(R * Tc, B).contiguous()
            outs = [torch.empty(R * Tc, B, dtype=torch.float64) for _ in range(2)]
            block_call(w, xc, R, Tc, B, H, P, dil, t0, after[0], outs[0])
            composed_call(w, xc, R, Tc, B, H, P, dil, t0, after[1], outs[1])
            assert torch.isfinite(outs[0]).all()
            steps[key] = (after, float((outs[0] - outs[1]).abs().max()))
        return steps[key]

    def walk(t0, rings):
        if t0 == T13:
            live = torch.arange(T13 - cap, T13) % cap                # every slot holds a frame by now
            tally["worst"] = max(tally["worst"], float((rings[0][:, live] - rings[1][:, live]).abs().max()))
            tally["chunkings"] += 1
            return
        for Tc in range(1, min(5, T13 - t0) + 1):
            after, err = step(t0, Tc, rings)
            tally["worst"] = max(tally["worst"], err)
            walk(t0 + Tc, after)

    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                         # thousands of tiny operations: a thread pool only waits
    try:
        walk(0, [torch.full((R, cap, H), float("nan"), dtype=torch.float64) for _ in range(2)])
    finally:
        torch.set_num_threads(threads)
    assert tally["chunkings"] == sum(1 for _ in compositions(T13)) > 3000 and tally["worst"] <= 1e-12, tally
    assert any(t0 + Tc > cap for t0, Tc, _, _ in steps) and any(t0 == 0 for t0, _, _, _ in steps)      # a wrap, a start


@pytest.mark.parametrize("with_rb", [True, False])
def test_rows_form_table_rules(with_rb):
    B, H, P, dil, E, nslots, Tc, A = 4, 8, 3, 2, 4, 5, 4, 5
    w = params(B, H, P, E, with_rb, nslots, seed=3)
    g = torch.Generator().manual_seed(4)
    cap = (P - 1) * dil + Tc
    SENT = -777.0
    ring0 = torch.randn(nslots, cap, H, dtype=torch.float64, generator=g)
    ring0[4] = SENT                                                  # slot 4 is named by no entry
    x = torch.randn(A, Tc, B, dtype=torch.float64, generator=g)
    slot = torch.tensor([3, 0, 9, 1, 2], dtype=torch.int32)          # row 2 names no slot
    t0 = torch.tensor([11, 0, 5, -1, 6], dtype=torch.int64)          # row 3 has a negative t0
    tc = torch.tensor([4, 2, 3, 2, 9], dtype=torch.int32)            # row 4 is clamped to Tc
    valid = [(0, 3, 11, 4), (1, 0, 0, 2), (4, 2, 6, 4)]

    def run(xin):
        ring, out = ring0.clone(), torch.full((A * Tc, B), float("nan"), dtype=torch.float64)
        emu_stream_block.tcn_block_stream_rows_fwd(xin.reshape(A * Tc, B), w["rb"], w["W1"], w["b1"], w["a1"], w["gamma1"],
                                                   w["beta1"], w["wd"], w["bd"], w["a2"], w["gamma2"], w["beta2"], w["W2"], w["b2"],
                                                   A, Tc, B, H, P, dil, EPS, slot, t0, tc, ring, out)
        return ring, out.reshape(A, Tc, B)

    ring, out = run(x)
    for i, sl, first, n in valid:                                    # each valid row is the solo form on that row
        r1, o1 = ring0[sl:sl + 1].clone(), torch.empty(n, B, dtype=torch.float64)
        block_call(w, x[i, :n].contiguous(), 1, n, B, H, P, dil, first, r1, o1, rb=None if w["rb"] is None else w["rb"][sl:sl + 1])
        assert torch.equal(out[i, :n], o1) and torch.equal(ring[sl], r1[0])
        assert torch.equal(out[i, n:], torch.zeros(Tc - n, B, dtype=torch.float64))
    for i in (2, 3):
        assert torch.equal(out[i], torch.zeros(Tc, B, dtype=torch.float64))
    assert torch.equal(ring[4], torch.full((cap, H), SENT, dtype=torch.float64))     # unnamed: untouched
    assert torch.equal(ring[1], ring0[1])                                             # named by a row with t0 < 0: untouched
    xp = x.clone()
    xp[1, 2:] = float("nan")                                         # behind tc
    xp[2], xp[3] = float("nan"), float("inf")                        # rows that are skipped
    ring_p, out_p = run(xp)
    assert torch.equal(out_p, out) and torch.equal(ring_p, ring)


# ---- the streamer on the emulation --------------------------------------------------------------------------------------
BLOCK_CONFIGS = ["multi_cln_concatconv", "multi_cln_joint_spexplus"]
_REF = {}


def _case(name):
    """(model, x, enrollment, whole-utterance estimate, fused=True stream) on the emulation: once per configuration."""
    if name not in _REF:
        from wesep_amd.streaming import ConvTasNetStreamer
        mp = pytest.MonkeyPatch()
        emu_stream_block.install(mp)
        mp.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
        model, x, enroll = make_fused_case(name, 2)
        st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, fused=True)
        st.enroll(enroll)
        _REF[name] = (model, x, enroll, whole(model, x, enroll), stream(st, x, chunkings()["all160"])[0])
        mp.undo()
    return _REF[name]


@pytest.mark.parametrize("chunking", ["all160", "all7", "random1to400", "one"])
@pytest.mark.parametrize("name", BLOCK_CONFIGS)
def test_block_streamer_matches_fused_and_forward(name, chunking, monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream_block.install(monkeypatch)
    monkeypatch.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
    model, x, enroll, ref, fused = _case(name)
    st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, block=True)
    st.enroll(enroll)
    got, _ = stream(st, x, chunkings()[chunking])
    assert got.shape == ref.shape == (2, ((T_TOTAL - 20) // 10) * 10 + 20) and float(ref.abs().max()) > 0
    ef, ew = rel(got, fused), rel(got, ref)
    print(f"block stream {name} {chunking}: rel L2 {ef:.3e} against fused=True, {ew:.3e} against the forward")
    assert ef < 1e-6 and ew < 1e-4, (name, chunking, ef, ew)


def test_block_is_one_dev_call_per_block_and_the_default_is_unchanged(monkeypatch):
    from wesep_amd.streaming import ConvTasNetStreamer
    model, x, enroll, _, _ = _case("multi_cln_concatconv")

    def names(**kw):
        record = []
        with monkeypatch.context() as mp:
            emu_stream_block.install(mp, record)
            mp.setattr("wesep_amd.functional_tasnet.SPK_MODE", None)
            st = ConvTasNetStreamer(model, 2, max_chunk_frames=64, **kw)
            st.enroll(enroll)
            del record[:]
            st.push(x[:, :400])                                      # 25 frames: one group
        return record

    default, fused, block = names(), names(fused=True), names(block=True)
    nblocks = SMALL["X"] * SMALL["R"]
    assert "tcn_block_stream_fwd" not in default + fused and default == names(fused=False, block=False)
    assert block.count("tcn_block_stream_fwd") == nblocks and "tcn_mid_stream_fwd" not in block
    assert len(fused) - len(block) == 2 * nblocks                    # GEMM, middle, GEMM -> one call


def test_block_refusals_by_message(monkeypatch):
    from wesep_amd import functional_tasnet as FT
    from wesep_amd.models import get_model
    from wesep_amd.streaming import ConvTasNetStreamer
    emu_stream_block.install(monkeypatch)
    bn = get_model("ConvTasNet")(**dict(SMALL, norm="BN")).eval()
    with pytest.raises(NotImplementedError, match="block=True is built for cLN blocks; this model's norm is 'BN'"):
        ConvTasNetStreamer(bn, 2, block=True)
    skip = get_model("ConvTasNet")(**dict(SMALL, norm="cLN", skip_con=True)).eval()
    with pytest.raises(NotImplementedError, match="block=True has no skip-connection branch"):
        ConvTasNetStreamer(skip, 2, block=True)
    ConvTasNetStreamer(skip, 2, fused=True)
    ConvTasNetStreamer(bn, 2)
    with pytest.raises(NotImplementedError, match="block=True is built for cLN"):        # before any argument is touched
        FT.conv_block_stream(torch.zeros(4, 8), None, (2, 2, "BN", 1, None), None, 0, *([None] * 12), block=True)
    with pytest.raises(NotImplementedError, match="skip-connection branch .wsc given."):
        FT.conv_block_stream(torch.zeros(4, 8), None, (2, 2, "cLN", 1, None), None, 0, *([None] * 12), wsc=torch.zeros(1),
                             block=True)
