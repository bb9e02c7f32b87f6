"""Whole-utterance inference / scoring loop on the MI355X engine -- the part of wesep/bin/infer.py
that touches the model (infer.py:72-73, 108-128, 150-175): eval mode, no_grad, batch of the two
target speakers of one mixture, variable length, peak normalisation to 0.9, SI-SNR / SI-SNRi.
Dataset / config / wav-file plumbing stays in wesep (it is not on the device path)."""
import numpy as np
import torch

from ..utils.score import cal_SISNRi


def peak_normalise_rows(outputs, lengths):
    """The rule of infer.py:118-128 for a ragged batch, row by row as if each were a batch of one: a row whose maximum over
    its valid part is positive is scaled to a peak of 0.9 over that part.  outputs: numpy [B, T] (zeros behind lengths[r])."""
    outputs = np.array(outputs, dtype=np.float32)
    for r, n in enumerate(lengths):
        row = outputs[r, :int(n)]
        if row.max() > 0:
            outputs[r, :int(n)] = row / np.abs(row).max() * 0.9
    return outputs


@torch.no_grad()
def extract(model, wav_mix, enroll, lengths=None, enroll_lengths=None):
    """wav_mix [B, T], enroll [B, spk_emb_dim] (device tensors) -> numpy [B, T], peak-normalised like
    infer.py:118-128 (only when every row's maximum is positive, exactly as the reference).
    lengths (B ints; pBSRNN): a ragged batch -- row r holds lengths[r] valid samples and comes out as that utterance alone
    would (model(..., lengths=)), normalised over its valid part (peak_normalise_rows), zeros behind it.
    enroll_lengths (B ints; joint pBSRNN): the valid samples (spk_feat=False) or frames (spk_feat=True) of every enrollment
    row -- the speaker encoder runs once over the rectangle (model(..., enroll_lengths=))."""
    model.eval()
    kw = {} if enroll_lengths is None else {"enroll_lengths": [int(n) for n in enroll_lengths]}
    if lengths is not None:
        outputs = model(wav_mix.float(), enroll.float(), lengths=[int(n) for n in lengths], **kw)
        return peak_normalise_rows((outputs[0] if isinstance(outputs, (list, tuple)) else outputs).cpu().numpy(), lengths)
    outputs = model(wav_mix.float(), enroll.float(), **kw)
    if isinstance(outputs, (list, tuple)):
        outputs = outputs[0]
    if torch.min(outputs.max(dim=1).values) > 0:
        outputs = outputs / outputs.abs().max(dim=1, keepdim=True)[0] * 0.9
    return outputs.cpu().numpy()


def extract_engine(engine, wav_mix, enroll, kind=None, lengths=None, window=None, overlap=None):
    """The same step on the native runtime (`wesep_amd.engine.Engine`, runtime/libwesep_engine.so): host arrays in,
    numpy [B, T] out, peak-normalised by the same rule.  `kind`: an `ENROLL_*` constant; default by rank
    (2-D embeddings for fixed-embedding models are ENROLL_EMBEDDING, 3-D is fbank; pass ENROLL_WAVE for audio).
    lengths (B ints): a ragged batch, as in extract (Engine.separate_ragged; the enrollment rows keep their full length).
    window (samples; overlap defaults to window // 4): long recordings -- every mixture goes through
    Engine.separate_long on its own (over its own samples when lengths is given), and the peak normalisation is applied
    to the assembled estimate, not per window."""
    from .. import engine as E
    wav_mix = np.ascontiguousarray(wav_mix, dtype=np.float32)
    enroll = np.ascontiguousarray(enroll, dtype=np.float32)
    if kind is None:
        kind = E.ENROLL_FBANK if enroll.ndim == 3 else E.ENROLL_EMBEDDING
    if window is not None:
        overlap = int(window) // 4 if overlap is None else overlap
        outputs = np.zeros_like(wav_mix)
        for r in range(wav_mix.shape[0]):
            n = wav_mix.shape[1] if lengths is None else int(lengths[r])
            outputs[r, :n] = engine.separate_long(wav_mix[r, :n], enroll[r:r + 1], kind, window, overlap)[0]
        if lengths is not None:
            return peak_normalise_rows(outputs, lengths)
    elif lengths is not None:
        rows = engine.separate_ragged([wav_mix[r, :int(n)] for r, n in enumerate(lengths)], list(enroll), kind)
        outputs = np.zeros_like(wav_mix)
        for r, row in enumerate(rows):
            outputs[r, :len(row)] = row
        return peak_normalise_rows(outputs, lengths)
    else:
        outputs = engine.separate(wav_mix, enroll, kind)
    if outputs.max(axis=1).min() > 0:
        outputs = outputs / np.abs(outputs).max(axis=1, keepdims=True) * 0.9
    return outputs


def evaluate(model, batches, device="cuda"):
    """batches: iterable of dicts with `wav_mix` [B, T], `wav_targets` [B, T], `spk_embeds` [B, E]
    (what tse_collate_fn_2spk yields, infer.py:108-116).  Returns (mean SI-SNR, mean SI-SNRi, count):
    the accumulation of infer.py:150-175.  A batch may carry `lengths` [B]: utterances of different lengths padded to
    one T (extract's ragged batch); every row is then scored over its own samples."""
    tot, toti, n = 0.0, 0.0, 0
    for b in batches:
        mix = torch.as_tensor(b["wav_mix"]).float().to(device)
        ref = np.asarray(b["wav_targets"], dtype=np.float32)
        lengths = b.get("lengths") if hasattr(b, "get") else None
        if lengths is not None:
            est = extract(model, mix, torch.as_tensor(b["spk_embeds"]).float().to(device), lengths=lengths)
        else:
            est = extract(model, mix, torch.as_tensor(b["spk_embeds"]).float().to(device))
        mixn = mix.cpu().numpy()
        for r in range(est.shape[0]):
            end = min(len(est[r]), len(ref[r]))
            if lengths is not None:
                end = min(end, int(lengths[r]))
            s, si = cal_SISNRi(est[r][:end], ref[r][:end], mixn[r][:end])
            tot, toti, n = tot + s, toti + si, n + 1
    return tot / max(n, 1), toti / max(n, 1), n
