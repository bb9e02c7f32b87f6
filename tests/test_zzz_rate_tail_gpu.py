"""GPU: the rate tail pool (runtime/rate_tail_pool.cc; ws_window_resample_rows_fwd of resample.hip; DESIGN 7 "Rate tail pool").
The gather kernel against the whole-signal resampler, bit for bit, and against the float64 reference; the pool on the tiny
containers of tests/test_zzz_tail_gpu.py against the chain of existing public pieces it replaces -- a streaming resampler in, a
tail pool at the container's rate, a streaming resampler per target back -- bit for bit."""
import numpy as np
import pytest
import torch

from tests import emu_rate_tail as RT
from tests import resample_contract as RC
from tests.test_longform_gpu import ENGINE_CASES, _cuda, _model
from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd import resample as RS
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
NAN = float("nan")
MODEL_RATE = 16000


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- the kernel ------------------------------------------------------------------------------------------------------
N_SIG = 3000
# (rate_in, first output q0 of the whole signal, L, fill, final); None: the last L outputs, so the row ends the signal
KERNEL_ROWS = [(8000, 1001, 257, 3, 0),          # starts at phase 1 of group 500; one workgroup and a bit, zeros behind
               (48000, 333, 600, 0, 0),          # several workgroups
               (44100, 0, 300, 0, 0),            # from sample 0: lead = w, the taps before the signal are skipped; global table
               (44100, None, 257, 3, 1),         # ends at the last output: taps behind the end are skipped; starts at phase 32
               (8000, None, 200, 0, 1),
               (16000, 123, 500, 5, 0)]          # the identity table


def _kernel_case(d, x, behind):
    """the arenas and the table of the one launch; `behind`: what follows every span's valid samples in the arena"""
    rows, bufs, tabs, expect = [], [], [], []
    buf_at, taps_at, out_at = 3, 1, 2                               # odd first offsets: no alignment is assumed
    for rate, q0, L, fill, final in KERNEL_ROWS:
        U, D, w, K = RT.geometry(rate, MODEL_RATE)
        n_out = RT.out_len(N_SIG, rate, MODEL_RATE)
        q0 = n_out - L if q0 is None else q0
        assert (q0 + L == n_out) == bool(final)
        g_a, g_last = q0 // U, (q0 + L - 1) // U
        lo, lead, g_first = (g_a * D - w, 0, 0) if g_a * D >= w else (0, w, g_a)
        hi = N_SIG if final else g_last * D - w + K
        assert 0 <= lo < hi <= N_SIG
        taps = np.ones(1, np.float32) if rate == MODEL_RATE else dev.resample_taps(rate, MODEL_RATE).reshape(-1)
        rows.append(dict(in_off=buf_at, taps_off=taps_at, out_off=out_at, U=U, D=D, K=K, lead=lead, n_valid=hi - lo, final=final,
                         g_first=g_first, p_first=q0 % U, L=L, fill=fill))
        bufs.append((buf_at, x[lo:hi]))
        tabs.append((taps_at, taps))
        expect.append((rate, q0))
        buf_at += hi - lo + 7                                       # (7 floats of `behind` after every span)
        taps_at += len(taps) + 1
        out_at += L + fill + 2
    buf = np.full(buf_at + 4, behind, np.float32)
    tab = np.full(taps_at + 4, NAN, np.float32)
    for o, v in bufs:
        buf[o:o + len(v)] = v
    for o, v in tabs:
        tab[o:o + len(v)] = v
    return rows, expect, torch.from_numpy(buf).to(d), torch.from_numpy(tab).to(d), torch.full((out_at + 4,), NAN, device=d)


def test_window_resample_rows_contract():
    d = _cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N_SIG, generator=g).numpy()
    xd = torch.from_numpy(x).to(d)[None]
    whole = {r: (xd[0].cpu().numpy() if r == MODEL_RATE else RS.resample(xd, r, MODEL_RATE)[0].cpu().numpy()) for r in {k[0] for k in KERNEL_ROWS}}
    ref64 = {r: RT.reference(x, r, MODEL_RATE) for r in whole}
    bound = {r: (np.zeros(N_SIG) if r == MODEL_RATE else RC.bound(x, r, MODEL_RATE)) for r in whole}
    assert RT.geometry(8000, MODEL_RATE)[0] * RT.geometry(8000, MODEL_RATE)[3] <= 2048 < np.prod(RT.geometry(44100, MODEL_RATE)[::3])   # both paths
    outs = []
    for behind in (NAN, 0.25):                                       # NaN behind n_valid changes nothing
        rows, expect, buf, tab, y = _kernel_case(d, x, behind)
        assert len(rows) == 6 and any(r["p_first"] % r["U"] for r in rows) and any(r["lead"] > 0 for r in rows)
        dev.window_resample_rows(rows, buf, tab, y)
        torch.cuda.synchronize()
        out = y.cpu().numpy()
        written = np.zeros(len(out), bool)
        worst = 0.0
        for r, (rate, q0) in zip(rows, expect):
            got = out[r["out_off"]:r["out_off"] + r["L"]]
            written[r["out_off"]:r["out_off"] + r["L"] + r["fill"]] = True
            # every row is bit for bit the slice of ws_resample_fwd on the whole signal ...
            assert _same_bits(got, whole[rate][q0:q0 + r["L"]]), (rate, q0)
            # ... within the bound of the float64 reference ...
            err, bd = np.abs(got.astype(np.float64) - ref64[rate][q0:q0 + r["L"]]), bound[rate][q0:q0 + r["L"]]
            assert (err <= bd).all(), (rate, q0, float(err.max()))
            worst = max(worst, float((err / np.maximum(bd, 1e-300)).max()))
            # ... with `fill` zeros behind it
            assert _same_bits(out[r["out_off"] + r["L"]:r["out_off"] + r["L"] + r["fill"]], np.zeros(r["fill"], np.float32))
        assert np.isnan(out[~written]).all()                          # nothing behind L + fill was written
        outs.append(out[written])
    assert _same_bits(outs[0], outs[1])
    print(f"ws_window_resample_rows_fwd: worst error {worst:.3f} of the bound gamma_K sum |taps| |x|")


# ---- engines -----------------------------------------------------------------------------------------------------------
WARM = {"pBSRNN": 1000, "ConvTasNet": 500, "DPCCN": 3968}
FADE, K_ = 128, 2
ARCHS = ("ConvTasNet", "DPCCN", "pBSRNN")


def _schedule(lens, rates, S, warm):
    """Rounds of a run: recording i is attached in round 2 i; every round pushes each recording in flight its next packet of 40 ms at
    its own rate (cut to what is left and to what the slot still takes) and ticks them all; a recording whose samples are used up
    is flushed and detached.  -> [(attach [i], {i: (pos, n)}, flush [i])], and per round the recordings that fire"""
    model, pos, rounds, fired = {}, {}, [], []
    todo, t = list(range(len(lens))), 0
    while todo or model:
        att = [i for i in todo if 2 * i <= t]
        for i in att:
            todo.remove(i)
            model[i], pos[i] = RT.Counts(S, FADE, warm, rates[i], MODEL_RATE), 0
        packets = {}
        for i, m in model.items():
            c = min(int(0.04 * rates[i] + 0.5), lens[i] - pos[i], m.room())
            assert c >= 1
            packets[i] = (pos[i], c)
            m.push(c)
            pos[i] += c
        fired.append([i for i, m in sorted(model.items()) if m.fires()])
        for m in model.values():
            m.tick()
        done = [i for i in model if pos[i] == lens[i]]
        for i in done:
            del model[i]
        rounds.append((att, packets, done))
        t += 1
    return rounds, fired


def _run_pool(c, max_rows, audio=None, split=1):
    """the rate tail pool; split: every packet goes in as `split` pushes between two ticks"""
    eng, audio = c["eng"], c["audio"] if audio is None else audio
    pool = eng.rate_tail_pool(len(audio), K_, c["S"], FADE, sorted(set(c["rates"])), c["warm"], max_rows)
    slot, parts = {}, {i: [] for i in range(len(audio))}
    for att, packets, done in c["rounds"]:
        for i in att:
            slot[i] = pool.attach(c["embs"][i], E.ENROLL_EMBEDDING, c["rates"][i])
        for j in range(split):
            cut = lambda n, j: (j * n // split, (j + 1) * n // split)
            chunks = {slot[i]: audio[i][p + cut(n, j)[0]:p + cut(n, j)[1]] for i, (p, n) in packets.items() if cut(n, j)[1] > cut(n, j)[0]}
            if chunks:
                pool.push(chunks)
        got = pool.tick([slot[i] for i in packets])
        for i in packets:
            if slot[i] in got:
                parts[i].append(got[slot[i]])
        for i in done:
            parts[i].append(pool.flush(slot[i]))
            pool.detach(slot.pop(i))
    pool.close()
    return [np.concatenate(p, axis=1) for p in parts.values()]


def _run_chain(c, max_rows):
    """The existing public pieces, chained: StreamResampler(r -> r0) fed the same packets; a tail pool at the container's rate fed
    its emissions and ticked at the same moments; one StreamResampler(r0 -> r) row per target; flushed in the same order and cropped
    to the samples pushed.  A recording at the container's rate is the plain tail pool fed its packets."""
    eng, audio, d = c["eng"], c["audio"], torch.device("cuda:0")
    pool = eng.tail_pool(len(audio), K_, c["S"], FADE, c["warm"], max_rows)
    slot, A, B, parts, back = {}, {}, {}, {i: [] for i in range(len(audio))}, {i: 0 for i in range(len(audio))}
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(d)
    down = lambda t: t.cpu().numpy()

    def through_b(i, v):
        if i in B and v.shape[1] > 0:
            v = down(B[i].push(up(v)))
        parts[i].append(v)
        back[i] += v.shape[1]

    for att, packets, done in c["rounds"]:
        for i in att:
            slot[i] = pool.attach(c["embs"][i], E.ENROLL_EMBEDDING)
            if c["rates"][i] != MODEL_RATE:
                A[i] = RS.StreamResampler(1, c["rates"][i], MODEL_RATE, max_push=8192, device=d)
                B[i] = RS.StreamResampler(K_, MODEL_RATE, c["rates"][i], max_push=8192, device=d)
        chunks = {}
        for i, (p, n) in packets.items():
            v = down(A[i].push(up(audio[i][p:p + n])[None]))[0] if i in A else audio[i][p:p + n]
            if len(v):
                chunks[slot[i]] = v
        if chunks:
            pool.push(chunks)
        got = pool.tick([slot[i] for i in packets])
        for i in packets:
            if slot[i] in got:
                through_b(i, got[slot[i]])
        for i in done:
            if i in A:
                v = down(A[i].flush())[0]
                if len(v):
                    pool.push({slot[i]: v})
            through_b(i, pool.flush(slot[i]))
            if i in B:
                v = down(B[i].flush())
                parts[i].append(v[:, :len(audio[i]) - back[i]])       # cropped to the samples pushed
            pool.detach(slot.pop(i))
    pool.close()
    return [np.concatenate(p, axis=1) for p in parts.values()]


@pytest.fixture(scope="module", params=ARCHS)
def rate_case(request, tmp_path_factory):
    """One engine; recordings at 8 / 16 / 48 kHz (and 44.1 kHz on pBSRNN) of about two and a half windows, attached two rounds
    apart, flushed at different rounds; the chain of existing pieces run once per max_rows: shared by the tests below."""
    _cuda()
    arch = request.param
    name, kw, _, S, _ = ENGINE_CASES[arch]
    path = str(tmp_path_factory.mktemp("ratetail") / f"{arch}.wsw")
    export_engine(_model(name, 11, joint_training=False, **kw), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(9)
    rates = [8000, 16000, 48000] + ([44100] if arch == "pBSRNN" else [])
    lens = [int((2.5 - 0.45 * i) * S * r / MODEL_RATE) + 1 for i, r in enumerate(rates)]
    audio = [(0.1 * torch.randn(m, generator=g)).numpy() for m in lens]
    embs = [torch.randn(K_, 256, generator=g).numpy() for _ in lens]
    c = dict(arch=arch, eng=eng, audio=audio, embs=embs, S=S, lens=lens, rates=rates, warm=WARM[arch])
    c["rounds"], c["fired"] = _schedule(lens, rates, S, c["warm"])
    c["chain"] = {}
    yield c
    eng.close()


def _chain(c, max_rows):
    if max_rows not in c["chain"]:
        c["chain"][max_rows] = _run_chain(c, max_rows)
    return c["chain"][max_rows]


@pytest.mark.parametrize("max_rows", [1, 8])
def test_rate_tail_pool_is_the_chain_of_existing_pieces(rate_case, max_rows):
    c = rate_case
    # the run asserts its own coverage: a tick fired three slots, the recordings are flushed in different rounds
    assert max(len(f) for f in c["fired"]) >= 3 and len({t for t, (_, _, done) in enumerate(c["rounds"]) if done}) >= 2, c["fired"]
    want = _chain(c, max_rows)
    got = _run_pool(c, max_rows)
    for i, n in enumerate(c["lens"]):
        assert got[i].shape == want[i].shape == (K_, n), (c["arch"], i, got[i].shape, want[i].shape)      # exactly the samples pushed
        assert np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        diff = float(np.abs(got[i].astype(np.float64) - want[i]).max())
        print(f"rate tail pool {c['arch']} max_rows {max_rows}, recording {i} at {c['rates'][i]} Hz: max |pool - chain| = {diff:.3e}")
        # (the recording at the container's rate: its chain IS the plain tail pool fed the same packets)
        assert _same_bits(got[i], want[i]), (c["arch"], max_rows, i, c["rates"][i], diff)
    assert c["eng"].info("cluster_fallbacks") == 0


def test_rate_tail_pool_does_not_depend_on_the_packet_split(rate_case):
    c = rate_case
    one, three = _run_pool(c, 8), _run_pool(c, 8, split=3)
    for i in range(len(c["lens"])):
        assert _same_bits(one[i], three[i]), (c["arch"], i)


def test_rate_tail_slots_do_not_depend_on_what_the_other_slots_carry(rate_case):
    """The same rounds -- so the same rows in every forward -- with the other recordings' audio replaced by NaN and inf: recording 0
    returns the same bits."""
    c = rate_case
    bad = []
    for x in c["audio"][1:]:
        y = x.copy()
        y[::7], y[3::11] = np.nan, np.inf
        bad.append(y)
    clean, dirty = _run_pool(c, 8), _run_pool(c, 8, audio=[c["audio"][0]] + bad)
    same, finite = _same_bits(dirty[0], clean[0]), bool(np.isfinite(dirty[0]).all())
    print(f"rate tail pool {c['arch']} max_rows 8, the other recordings fed NaN / inf: recording 0 {'keeps' if same else 'CHANGES'} its bits"
          f"{'' if finite else ' (not finite)'}")
    assert same and finite, c["arch"]
    assert not _same_bits(dirty[1], clean[1])                      # (the other data did reach its own slot)


def test_rate_tail_pool_launches_on_the_device(rate_case):
    """One tick of three slots at three rates, each with all a window lets it push: the forwards of a plain tail pool with these
    window lengths and three launches more, one copy -- and nothing when nothing fires."""
    from tests import emu_tail as T
    c = rate_case
    eng, S = c["eng"], c["S"]
    pool = eng.rate_tail_pool(3, K_, S, FADE, [8000, 48000], c["warm"], max_rows=8)
    slots = [pool.attach(c["embs"][i], E.ENROLL_EMBEDDING, c["rates"][i]) for i in range(3)]
    rooms = [pool.room(s) for s in slots]
    assert rooms == [S // 2, S, 3 * S]
    pool.push({s: c["audio"][i][:rooms[i]] for i, s in enumerate(slots)})
    out = pool.tick()
    n_tick, n_fw = eng.info("n_launches"), eng.info("rate_tail_pool_forwards")
    lengths = [RT.emitted(n, r, MODEL_RATE) for n, r in zip(rooms, c["rates"][:3])]
    assert lengths == [S - 14, S, S - 7] and eng.info("rate_tail_pool_rows") == 3 * K_ and sorted(out) == slots
    counts = []
    for rows, L in T.tick_forwards(lengths, K_, S, 8):                # a forward's rectangular count, from ws_engine_separate itself
        eng.separate(np.zeros((rows, L), np.float32), np.zeros((rows, 256), np.float32), E.ENROLL_EMBEDDING)
        counts.append(eng.info("n_launches"))
    assert n_fw == len(counts) == 3 and n_tick == E.rate_tail_launches(counts)
    assert pool.tick() == {} and eng.info("n_launches") == 0         # nothing new: no slot fires
    pool.close()
