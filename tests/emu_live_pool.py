"""numpy restatement of the live pool (include/wesep_hip.h: ws_window_slots_fwd, ws_xfade_stream_rows_fwd; include/wesep_engine.h:
ws_engine_live_pool_*; DESIGN 7 "Live pool"), written from the headers on top of tests/emu_live.py: the two table-driven
kernels over flat arenas, and the round rule around them with the separator replaced by a function of (window index, samples)
per slot.  Offsets count elements into 1-D arrays, as the kernels' offsets count floats into their arenas.
  round   in ascending slot order every slot that still owes windows gives min(owed, g_max, cap - Wr % cap) consecutive
          windows; the round's rows are ordered (slot, target, window) and go through the separator in forwards of at most
          max_rows rows; one gather, one scatter into the rings, one cross-fade per round."""
import numpy as np

from tests import emu_live as M

ROUND_LAUNCHES = 3      # WS_LIVE_POOL_ROUND_LAUNCHES


def window_slots(rows, src, dst):
    """ws_window_slots_fwd: rows of (src_off, dst_off, len, scale); dst[dst_off + j] = src[src_off + j] * scale, rounded to dst's
    dtype.  The refusals of the entry point are assertions."""
    assert 1 <= len(rows) <= 65535
    spans = []
    for i, (so, do, ln, sc) in enumerate(rows):
        assert ln >= 1 and 0 <= so <= len(src) - ln and 0 <= do <= len(dst) - ln, f"row {i} leaves its arena"
        spans.append((do, do + ln, i))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], f"row {b[2]}: its dst range overlaps the dst range of row {a[2]}"
    for so, do, ln, sc in rows:
        dst[do:do + ln] = (src[so:so + ln] * dst.dtype.type(sc)).astype(dst.dtype)


def xfade_stream_rows(rows, S, O, cap, ring, scale_ring, out):
    """ws_xfade_stream_rows_fwd: rows of dicts (ring_off, scale_off (-1: none), out_off, i0, count, windows_run, final, W, n); row
    i is emu_live.xfade_stream with K = 1 on the ring [cap][S] at ring_off.  A row with count == 0 is skipped."""
    assert 1 <= len(rows) <= 65535
    spans = []
    for i, r in enumerate(rows):
        assert 0 <= r["ring_off"] <= len(ring) - cap * S, f"row {i}: ring leaves its arena"
        assert r["scale_off"] == -1 or 0 <= r["scale_off"] <= len(scale_ring) - cap, f"row {i}: scale_ring leaves its arena"
        if r["count"]:
            assert 0 <= r["out_off"] <= len(out) - r["count"], f"row {i}: out leaves its arena"
            spans.append((r["out_off"], r["out_off"] + r["count"], i))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], f"row {b[2]}: its out range overlaps the out range of row {a[2]}"
    for r in rows:
        if not r["count"]:
            continue
        rg = ring[r["ring_off"]:r["ring_off"] + cap * S].reshape(1, cap, S)
        sc = None if r["scale_off"] < 0 else scale_ring[r["scale_off"]:r["scale_off"] + cap]
        final = (r["W"], r["n"]) if r["final"] else None
        out[r["out_off"]:r["out_off"] + r["count"]] = M.xfade_stream(rg, S, O, r["i0"], r["count"], r["windows_run"], final, sc)[0]


class _Slot:
    def __init__(self, sep, scale, dtype):
        self.sep, self.scale = sep, scale
        self.pend, self.base, self.N, self.Wr, self.E, self.done = np.zeros(0, dtype), 0, 0, 0, 0, False


class Pool:
    """The round rule.  attach(separate, scale) takes the lowest free slot -- `separate(w, x [L]) -> [K][L]` stands for the
    separator with the slot's enrollments, one row of it per target; `scale(w)` for TF-GridNet's per-window factor (the
    gather multiplies by 1 / scale(w) and the separator's stand-in is given the samples times scale(w) again, so it sees
    emu_live.Live's samples exactly when the factors are powers of two) -- and
    push({slot: chunk}) / flush(slot) return [K][m] per slot.  A slot's rings are re-poisoned with NaN at attach and a ring
    slot that receives a window is NaN behind its L samples, so a read outside the contract shows.  rounds: per round of the
    last call the list of its forwards' row counts."""

    def __init__(self, slots, K, S, O, max_rows, dtype=np.float64):
        self.slots, self.K, self.S, self.O, self.H, self.max_rows = slots, K, S, O, S - O, max_rows
        self.g_max = max(1, max_rows // K)
        self.cap, self.dtype = self.g_max + 3, dtype
        self.ring = np.full(slots * K * self.cap * S, np.nan, dtype)
        self.scale_ring = np.full(slots * self.cap, np.nan, dtype)
        self.sl = [None] * slots
        self.rounds = []

    def attach(self, separate, scale=None):
        i = self.sl.index(None)          # a full pool: ValueError
        self.sl[i] = _Slot(separate, scale, self.dtype)
        n = self.K * self.cap * self.S
        self.ring[i * n:(i + 1) * n] = np.nan
        self.scale_ring[i * self.cap:(i + 1) * self.cap] = np.nan
        return i

    def detach(self, i):
        assert self.sl[i] is not None
        self.sl[i] = None

    def _round(self, parts, out):
        """parts: dicts (slot, w0, g, L, a: offset of the span in the slot's pending samples, fade: the slot's cross-fade row
        without ring_off / scale_off / out_off, out_off, ld)"""
        K, S, H, cap = self.K, self.S, self.H, self.cap
        span, gather, meta = [], [], []
        for p in parts:
            sl, g, L = self.sl[p["slot"]], p["g"], p["L"]
            if g:
                at = sum(len(s) for s in span)
                span.append(sl.pend[p["a"]:p["a"] + (g - 1) * H + L])
                for k in range(K):
                    for w in range(g):
                        r = len(gather)
                        inv = 1.0 if sl.scale is None else 1.0 / sl.scale(p["w0"] + w)
                        gather.append((at + w * H, r * L, L, inv))
                        meta.append((p["slot"], k, p["w0"] + w, L))
        forwards = []
        if gather:
            src = np.concatenate(span)
            L = meta[0][3]
            rows = np.full(len(gather) * L, np.nan, self.dtype)
            window_slots(gather, src, rows)
            y = np.full(len(gather) * L, np.nan, self.dtype)
            for r0 in range(0, len(gather), self.max_rows):              # forwards of at most max_rows rows, whichever slots
                rs = range(r0, min(r0 + self.max_rows, len(gather)))
                for r in rs:
                    slot, k, w, _ = meta[r]
                    sl = self.sl[slot]
                    x = rows[r * L:(r + 1) * L]
                    y[r * L:(r + 1) * L] = sl.sep(w, x if sl.scale is None else x * sl.scale(w))[k]
                forwards.append(len(rs))
            for r, (slot, k, w, _) in enumerate(meta):                   # the scatter into the rings
                o = ((slot * K + k) * cap + w % cap) * S
                self.ring[o:o + S] = np.nan
                self.ring[o:o + L] = y[r * L:(r + 1) * L]
                if self.sl[slot].scale is not None:
                    self.scale_ring[slot * cap + w % cap] = self.sl[slot].scale(w)
        fade = []
        for p in parts:
            for k in range(K):
                fade.append(dict(p["fade"], ring_off=(p["slot"] * K + k) * cap * S,
                                 scale_off=-1 if self.sl[p["slot"]].scale is None else p["slot"] * cap,
                                 out_off=p["out_off"] + k * p["ld"]))
        xfade_stream_rows(fade, S, self.O, cap, self.ring, self.scale_ring, out)
        self.rounds.append(forwards)

    def push(self, chunks):
        S, H, K = self.S, self.H, self.K
        ids = sorted(chunks)
        target, e0, base, total = {}, {}, {}, 0
        for i in ids:
            sl = self.sl[i]
            assert sl is not None and not sl.done and len(chunks[i]) >= 1
            sl.pend = np.concatenate([sl.pend, np.asarray(chunks[i], self.dtype)])
            sl.N += len(chunks[i])
            target[i], e0[i], base[i] = M.windows_run(sl.N, S, H), sl.E, total
            total += K * (M.emitted(sl.N, S, H) - sl.E)
        out = np.full(total, np.nan, self.dtype)
        self.rounds = []
        while True:
            parts = []
            for i in ids:
                sl = self.sl[i]
                if sl.Wr >= target[i]:
                    continue
                g = min(target[i] - sl.Wr, self.g_max, self.cap - sl.Wr % self.cap)
                run, ld = sl.Wr + g, M.emitted(sl.N, S, H) - e0[i]
                parts.append(dict(slot=i, w0=sl.Wr, g=g, L=S, a=sl.Wr * H - sl.base, ld=ld, out_off=base[i] + sl.E - e0[i],
                                  fade=dict(i0=sl.E, count=(run - 1) * H - sl.E, windows_run=run, final=0, W=0, n=0)))
            if not parts:
                break
            self._round(parts, out)
            for p in parts:
                sl = self.sl[p["slot"]]
                sl.Wr = p["fade"]["windows_run"]
                sl.E = (sl.Wr - 1) * H
        res = {}
        for i in ids:
            sl = self.sl[i]
            m = sl.E - e0[i]
            res[i] = out[base[i]:base[i] + K * m].reshape(K, m)
            sl.pend, sl.base = sl.pend[sl.E - sl.base:], sl.E
            assert len(sl.pend) < S + H
        return res

    def flush(self, i):
        S, H, K = self.S, self.H, self.K
        sl = self.sl[i]
        assert sl is not None and not sl.done and sl.N >= 1
        n, m = sl.N, sl.N - sl.E
        p = dict(slot=i, w0=sl.Wr, g=0, L=S, a=0, ld=m, out_off=0)
        W = sl.Wr
        if n < S:
            p.update(g=1, w0=0, L=n, a=0)
            W = 1
        elif (n - S) % H:
            p.update(g=1, a=n - S - sl.base)
            W = sl.Wr + 1
        p["fade"] = dict(i0=sl.E, count=m, windows_run=W, final=1, W=W, n=n)
        out = np.full(K * m, np.nan, self.dtype)
        self.rounds = []
        self._round([p], out)
        sl.Wr, sl.E, sl.done = W, n, True
        return out.reshape(K, m)


def launches(rounds, plan):
    """the documented "n_launches" of a push: rounds as Pool.rounds, plan(rows) the rectangular plan's count"""
    return sum(sum(plan(f) for f in fw) + ROUND_LAUNCHES for fw in rounds) + 1
