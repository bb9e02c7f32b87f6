"""numpy restatement of the live pool's store / run / due (include/wesep_engine.h: ws_engine_live_pool_store, _run, _due; DESIGN 7
"Live pool"), written from the header on top of tests/emu_live_pool.py: the same two table-driven kernels and the same round
rule, with the packets stored first and the windows run when the caller says so.
  store   appends; refused (AssertionError) when a slot would hold STORE_LIMIT = 2 S + H or more pending samples.
  run     per named slot every complete window that has not run, by the round rule of a push; a slot in `final` then gives the
          end of its recording in the round after its last regular window: the end-aligned last window is a row of S samples
          among the others', a short recording (n < S) gets forwards of its own rows behind the round's rows of S samples.
  due     (K x complete windows not run, the largest N - (w H + S) over the slots' oldest such windows w)."""
import numpy as np

from tests import emu_live as M
from tests import emu_live_pool as P


def store_limit(S, H):
    return 2 * S + H      # WS_LIVE_POOL_STORE_LIMIT


def run_cap(S, H):
    return 2 * S + H      # WS_LIVE_POOL_RUN_CAP


class Pool(P.Pool):
    """emu_live_pool.Pool with store(), run() and due().  push(c) is store(c) + run(slots of c) and flush(i) is run([i], final=[i])
    by construction; rounds is that of the last call, as in the parent."""

    def _round(self, parts, out):
        """the parent's round for parts of one length; parts of other lengths (short final recordings) come behind them, each in
        forwards of its own rows"""
        K, S, H, cap = self.K, self.S, self.H, self.cap
        parts = [p for p in parts if not p["g"] or p["L"] == S] + [p for p in parts if p["g"] and p["L"] != S]
        span, gather, meta, segs, at = [], [], [], [], 0
        for p in parts:
            sl, g, L = self.sl[p["slot"]], p["g"], p["L"]
            if g:
                a0 = sum(len(s) for s in span)
                span.append(sl.pend[p["a"]:p["a"] + (g - 1) * H + L])
                if L == S and segs:
                    segs[-1][1] += K * g
                else:
                    segs.append([len(gather), K * g])
                for k in range(K):
                    for w in range(g):
                        inv = 1.0 if sl.scale is None else 1.0 / sl.scale(p["w0"] + w)
                        gather.append((a0 + w * H, at, L, inv))
                        meta.append((p["slot"], k, p["w0"] + w, L, at))
                        at += L
        forwards = []
        if gather:
            src = np.concatenate(span)
            rows = np.full(at, np.nan, self.dtype)
            P.window_slots(gather, src, rows)
            y = np.full(at, np.nan, self.dtype)
            for r0, n_rows in segs:
                for f0 in range(r0, r0 + n_rows, self.max_rows):
                    rs = range(f0, min(f0 + self.max_rows, r0 + n_rows))
                    assert len({meta[r][3] for r in rs}) == 1          # one length a forward
                    for r in rs:
                        slot, k, w, L, o = meta[r]
                        sl = self.sl[slot]
                        x = rows[o:o + L]
                        y[o:o + L] = sl.sep(w, x if sl.scale is None else x * sl.scale(w))[k]
                    forwards.append(len(rs))
            for slot, k, w, L, o in meta:
                d = ((slot * K + k) * cap + w % cap) * S
                self.ring[d:d + S] = np.nan
                self.ring[d:d + L] = y[o:o + L]
                if self.sl[slot].scale is not None:
                    self.scale_ring[slot * cap + w % cap] = self.sl[slot].scale(w)
        fade = []
        for p in parts:
            for k in range(K):
                fade.append(dict(p["fade"], ring_off=(p["slot"] * K + k) * cap * S,
                                 scale_off=-1 if self.sl[p["slot"]].scale is None else p["slot"] * cap,
                                 out_off=p["out_off"] + k * p["ld"]))
        P.xfade_stream_rows(fade, S, self.O, cap, self.ring, self.scale_ring, out)
        self.rounds.append(forwards)

    def store(self, chunks):
        for i in sorted(chunks):
            sl = self.sl[i]
            assert sl is not None and not sl.done and len(chunks[i]) >= 1
            assert len(sl.pend) + len(chunks[i]) < store_limit(self.S, self.H), "run first"
        for i in sorted(chunks):
            sl = self.sl[i]
            sl.pend = np.concatenate([sl.pend, np.asarray(chunks[i], self.dtype)])
            sl.N += len(chunks[i])
        self.rounds = []

    def due(self):
        S, H = self.S, self.H
        windows, age = 0, 0
        for sl in self.sl:
            if sl is None or sl.done:
                continue
            ready = M.windows_run(sl.N, S, H) - sl.Wr
            if ready > 0:
                windows += ready
                age = max(age, sl.N - (sl.Wr * H + S))
        return self.K * windows, age

    def run(self, slots, final=()):
        S, H, K = self.S, self.H, self.K
        ids = sorted(slots)
        target, e0, base, ld, total, ended = {}, {}, {}, {}, 0, set()
        for i in ids:
            sl = self.sl[i]
            assert sl is not None and not sl.done
            assert i not in final or sl.N >= 1, "nothing was pushed"
            target[i], e0[i], base[i] = M.windows_run(sl.N, S, H), sl.E, total
            ld[i] = (sl.N if i in final else M.emitted(sl.N, S, H)) - sl.E
            assert ld[i] <= run_cap(S, H)
            total += K * ld[i]
        out = np.full(total, np.nan, self.dtype)
        self.rounds = []
        while True:
            parts = []
            for i in ids:
                sl = self.sl[i]
                p = dict(slot=i, w0=sl.Wr, g=0, L=S, a=0, ld=ld[i], out_off=base[i] + sl.E - e0[i])
                if sl.Wr < target[i]:
                    g = min(target[i] - sl.Wr, self.g_max, self.cap - sl.Wr % self.cap)
                    run = sl.Wr + g
                    p.update(g=g, a=sl.Wr * H - sl.base,
                             fade=dict(i0=sl.E, count=(run - 1) * H - sl.E, windows_run=run, final=0, W=0, n=0))
                elif i in final and i not in ended:
                    n, W = sl.N, sl.Wr
                    if n < S:
                        p.update(g=1, w0=0, L=n, a=0)
                        W = 1
                    elif (n - S) % H:
                        p.update(g=1, a=n - S - sl.base)
                        W = sl.Wr + 1
                    p["fade"] = dict(i0=sl.E, count=n - sl.E, windows_run=W, final=1, W=W, n=n)
                else:
                    continue
                parts.append(p)
            if not parts:
                break
            self._round(parts, out)
            for p in parts:
                sl = self.sl[p["slot"]]
                sl.Wr = p["fade"]["windows_run"]
                if p["fade"]["final"]:
                    sl.E = sl.N
                    ended.add(p["slot"])
                else:
                    sl.E = (sl.Wr - 1) * H
        res = {}
        for i in ids:
            sl = self.sl[i]
            res[i] = out[base[i]:base[i] + K * ld[i]].reshape(K, ld[i])
            if i in final:
                sl.done = True
            else:
                sl.pend, sl.base = sl.pend[sl.E - sl.base:], sl.E
        return res

    def push(self, chunks):
        for i in sorted(chunks):                # (a push is not bounded by the store limit)
            sl = self.sl[i]
            assert sl is not None and not sl.done and len(chunks[i]) >= 1
            sl.pend = np.concatenate([sl.pend, np.asarray(chunks[i], self.dtype)])
            sl.N += len(chunks[i])
        return self.run(list(chunks))

    def flush(self, i):
        return self.run([i], final=[i])[i]
