"""Scores of the recipe's results, computed on the device: the unit error rate of normalisation and the word / character error
rate of a vocoder -> ASR loop.

Both are a unit-cost Levenshtein distance over integer sequences (dn_edit_distance of libdiffnorm_hip.so: one wavefront per pair,
csrc/metrics.hip), units after run-length de-duplication (dn_reduce_units, the device form of normalize.reduce_token).  They
replace the `editdistance.eval` calls of fairseq's WER scorer (fairseq/scoring/wer.py:50-58) and the per-utterance loop of
diff_norm_synthesis.py:25-46.  Substitution / insertion / deletion counts, alignments, weighted costs and BLEU are not done here.
Everything is integer arithmetic: a result is exact, and depends on the pair alone."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib

MAX_LEN = _lib.EDIT_DISTANCE_MAX_LEN  # tokens of a row dn_edit_distance takes


def _host_rows(name: str, rows, lengths):
    """Host input of one side -> (int32 [B, ld] CPU tensor, list of lengths), every length checked by name."""
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 2 or rows.dtype.is_floating_point:
            raise ValueError(f"{name}: an integer [B, ld] tensor or a list of sequences is expected, got {tuple(rows.shape)} {rows.dtype}")
        if lengths is None:
            raise ValueError(f"{name}_len: a padded tensor needs its rows' lengths")
        lens = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        ld = int(rows.shape[1])
    else:
        rows = [list(r) for r in rows]
        lens = [len(r) for r in rows] if lengths is None else [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        ld = max([len(r) for r in rows] + [1])
    if len(lens) != len(rows):
        raise ValueError(f"{name}_len: {len(lens)} lengths for {len(rows)} rows")
    for i, n in enumerate(lens):
        if n < 0:
            raise ValueError(f"{name}_len[{i}] = {n}: a length cannot be negative")
        if n > MAX_LEN:
            raise ValueError(f"{name}_len[{i}] = {n}: rows hold at most {MAX_LEN} tokens")
        if n > (ld if isinstance(rows, torch.Tensor) else len(rows[i])):
            raise ValueError(f"{name}_len[{i}] = {n} exceeds the leading dimension {ld if isinstance(rows, torch.Tensor) else len(rows[i])} of its row")
    if isinstance(rows, torch.Tensor):
        return rows.to(torch.int32), lens
    out = torch.zeros(len(rows), ld, dtype=torch.int32)
    for i, r in enumerate(rows):
        if r:
            out[i, : len(r)] = torch.tensor(r, dtype=torch.int32)
    return out, lens


def _check_ld(name: str, t: torch.Tensor):
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: a [B, ld] tensor with B >= 1 is expected, got {tuple(t.shape)}")
    if t.shape[1] > MAX_LEN:
        raise ValueError(f"{name}: rows of {t.shape[1]} tokens: rows hold at most {MAX_LEN} tokens")


def _upload(parts: Sequence[torch.Tensor], device) -> List[torch.Tensor]:
    """int32 CPU tensors -> their device copies through ONE pinned staging buffer and one async copy (as assemble_batch stages)."""
    sizes = [p.numel() for p in parts]
    stage = torch.empty(max(sum(sizes), 1), dtype=torch.int32).pin_memory()
    at = 0
    for p, n in zip(parts, sizes):
        stage[at: at + n] = p.reshape(-1)
        at += n
    dev = stage.to(device, non_blocking=True)
    out, at = [], 0
    for p, n in zip(parts, sizes):
        out.append(dev[at: at + n].view(p.shape))
        at += n
    return out


def _sides(sides, device):
    """[(name, rows, lengths)] -> device int32 tensors [rows, lengths, rows, lengths, ...]: every host side is checked first (nothing
    is launched or uploaded for a refused call), then all of them go up in one copy; device sides are taken as they are, their lengths
    clamped to [0, ld] by the kernels."""
    from .engine import _require_cuda

    host, out = {}, [None] * (2 * len(sides))
    for i, (name, rows, lengths) in enumerate(sides):
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            _check_ld(name, rows)
            if lengths is None:
                raise ValueError(f"{name}_len: a padded tensor needs its rows' lengths")
            device = rows.device if device is None else device
        else:
            t, lens = _host_rows(name, rows, lengths)
            _check_ld(name, t)
            host[i] = (t if t.shape[1] else t.new_zeros(t.shape[0], 1), torch.tensor(lens, dtype=torch.int32))
    device = _require_cuda("cuda:0" if device is None else device)
    if host:
        up = _upload([p for i in sorted(host) for p in host[i]], device)
        for k, i in enumerate(sorted(host)):
            out[2 * i], out[2 * i + 1] = up[2 * k], up[2 * k + 1]
    for i, (name, rows, lengths) in enumerate(sides):
        if i not in host:
            out[2 * i] = rows.to(device, torch.int32).contiguous()
            out[2 * i + 1] = torch.as_tensor(lengths).to(device, torch.int32).contiguous()
            if out[2 * i].shape[1] == 0:
                out[2 * i] = out[2 * i].new_zeros(out[2 * i].shape[0], 1)
    for i, (name, _, _) in enumerate(sides):
        if out[2 * i + 1].shape != (out[2 * i].shape[0],):
            raise ValueError(f"{name}_len: shape {tuple(out[2 * i + 1].shape)} for {out[2 * i].shape[0]} rows")
    return out, device


def edit_distance(a, b, a_len=None, b_len=None, device=None, panel_cols: int = 0) -> torch.Tensor:
    """Levenshtein distance (substitution, insertion, deletion cost 1 each) of B pairs -> int32 [B] on the device.

    a, b: device int tensors [B, lda] / [B, ldb] with a_len / b_len [B] (elements at or behind a length are never read), or host
    tensors, or lists of sequences (their own lengths when a_len / b_len are unset): host data goes up through one pinned staging
    buffer.  Rows hold at most 8192 tokens.  Host lengths are checked here -- above 8192, negative, above the leading dimension:
    each refused by name before anything is launched; device lengths are clamped to [0, ld] by the kernel.  `panel_cols` (0, or a
    multiple of 64 up to 2048) sweeps every pair in panels of that many columns through the workspace row: the same numbers,
    for tests."""
    (a, a_len, b, b_len), device = _sides([("a", a, a_len), ("b", b, b_len)], device)
    B = a.shape[0]
    if b.shape[0] != B:
        raise ValueError(f"edit_distance: {B} rows of a against {b.shape[0]} rows of b")
    lib = _lib.load()
    dist = torch.empty(B, dtype=torch.int32, device=device)
    nbytes = lib.dn_edit_distance_workspace_bytes(B, a.shape[1], b.shape[1])
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.dn_edit_distance(a.data_ptr(), a.shape[1], a_len.data_ptr(), b.data_ptr(), b.shape[1], b_len.data_ptr(), B, dist.data_ptr(),
                                        int(panel_cols), ws.data_ptr(), ws.numel() * 4, _lib.current_stream()), "dn_edit_distance")
    return dist


def reduce_units(units, lengths=None, device=None):
    """Run-length de-duplication of B rows on the device (normalize.reduce_token is the host definition) -> (reduced int32 [B, ld]
    with zeros at and behind reduced_len[b], reduced_len int32 [B], durations int32 [B, ld], first int32 [B, ld]: the index of each
    run's first frame).  units: a device or host int tensor [B, ld] with lengths [B], or a list of sequences."""
    if isinstance(units, torch.Tensor) and units.is_cuda:
        if units.dim() != 2 or units.shape[0] < 1 or lengths is None:
            raise ValueError("units: a [B, ld] tensor with B >= 1 and its lengths are expected")
        from .engine import _require_cuda

        device = _require_cuda(units.device if device is None else device)
        u = units.to(device, torch.int32).contiguous()
        ln = torch.as_tensor(lengths).to(device, torch.int32).contiguous()
        if u.shape[1] == 0:
            u = u.new_zeros(u.shape[0], 1)
    else:
        (u, ln), device = _sides([("units", units, lengths)], device)
    B, ld = u.shape
    red, dur, first = (torch.empty(B, ld, dtype=torch.int32, device=device) for _ in range(3))
    rlen = torch.empty(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().dn_reduce_units(u.data_ptr(), ln.data_ptr(), B, ld, red.data_ptr(), rlen.data_ptr(), dur.data_ptr(), first.data_ptr(),
                                               _lib.current_stream()), "dn_reduce_units")
    return red, rlen, dur, first


@dataclass
class ErrorRate:
    """Per-item edit-distance `errors` with the items' reference and hypothesis lengths; rate = total errors / total reference length."""
    errors: List[int]
    ref_len: List[int]
    hyp_len: List[int]

    def __post_init__(self):
        self.errors, self.ref_len, self.hyp_len = ([int(v) for v in x] for x in (self.errors, self.ref_len, self.hyp_len))
        if not len(self.errors) == len(self.ref_len) == len(self.hyp_len):
            raise ValueError(f"ErrorRate: {len(self.errors)} errors, {len(self.ref_len)} reference and {len(self.hyp_len)} hypothesis lengths")

    @property
    def total_errors(self) -> int:
        return sum(self.errors)

    @property
    def total_ref_len(self) -> int:
        return sum(self.ref_len)

    @property
    def total_hyp_len(self) -> int:
        return sum(self.hyp_len)

    @property
    def rate(self) -> float:
        if self.total_ref_len == 0:
            raise ValueError("ErrorRate: the references are empty: there is no length to divide by")
        return self.total_errors / self.total_ref_len

    @property
    def item_rates(self) -> List[float]:
        """errors / reference length per item; with an empty reference 0.0 for an empty hypothesis and inf otherwise."""
        return [e / r if r else (0.0 if h == 0 else float("inf")) for e, r, h in zip(self.errors, self.ref_len, self.hyp_len)]


def _error_rate(dist: torch.Tensor, hyp_len: torch.Tensor, ref_len: torch.Tensor) -> ErrorRate:
    d, h, r = torch.stack([dist, hyp_len.to(dist.device, torch.int32), ref_len.to(dist.device, torch.int32)]).cpu().tolist()  # one copy back
    return ErrorRate(d, r, h)


def unit_error_rate(hyp_units, ref_units, reduce: bool = True, hyp_len=None, ref_len=None, device=None) -> ErrorRate:
    """Edit distance between unit sequences (lists of sequences, or padded tensors with hyp_len / ref_len), by default after
    run-length de-duplication of BOTH sides on the device; rate = errors / reference units (after the reduction)."""
    (h, hl, r, rl), device = _sides([("hyp_units", hyp_units, hyp_len), ("ref_units", ref_units, ref_len)], device)
    if h.shape[0] != r.shape[0]:
        raise ValueError(f"unit_error_rate: {h.shape[0]} hypotheses against {r.shape[0]} references")
    if reduce:
        h, hl, _, _ = reduce_units(h, hl)
        r, rl, _, _ = reduce_units(r, rl)
    hl, rl = hl.clamp(0, h.shape[1]), rl.clamp(0, r.shape[1])
    return _error_rate(edit_distance(h, r, hl, rl), hl, rl)


def word_ids(hyps: Sequence[str], refs: Sequence[str]):
    """str.split() tokens -> int32 ids through ONE dictionary over the batch (first occurrence first) -> (hyp rows, ref rows)."""
    table = {}
    rows = [[table.setdefault(w, len(table)) for w in s.split()] for s in list(hyps) + list(refs)]
    return rows[: len(hyps)], rows[len(hyps):]


def char_ids(hyps: Sequence[str], refs: Sequence[str]):
    """Unicode code points of every string (a character outside the BMP is one id, a combining sequence is several)."""
    return [[ord(c) for c in s] for s in hyps], [[ord(c) for c in s] for s in refs]


def _text_rate(name, ids, hyps, refs, device) -> ErrorRate:
    if isinstance(hyps, str) or isinstance(refs, str):
        raise ValueError(f"{name}: lists of strings are expected, not one string")
    if len(hyps) != len(refs):
        raise ValueError(f"{name}: {len(hyps)} hypotheses against {len(refs)} references")
    if not len(hyps):
        return ErrorRate([], [], [])
    h, r = ids(hyps, refs)
    return _error_rate(edit_distance(h, r, device=device), torch.tensor([len(x) for x in h]), torch.tensor([len(x) for x in r]))


def wer(hyps: Sequence[str], refs: Sequence[str], device=None) -> ErrorRate:
    """Word error rate: the distance between the str.split() tokens of each hypothesis and its reference, on the device; only the
    mapping of words to ids runs on the host.  Case, punctuation and any other text normalisation are left to the caller."""
    return _text_rate("wer", word_ids, hyps, refs, device)


def cer(hyps: Sequence[str], refs: Sequence[str], device=None) -> ErrorRate:
    """Character error rate over Unicode code points, spaces included; case and punctuation are left to the caller, as in `wer`."""
    return _text_rate("cer", char_ids, hyps, refs, device)


def unit_changes(pred: Sequence[torch.Tensor], ref_units: torch.Tensor, ref_len: torch.Tensor):
    """normalize()'s hook: pred = the batch's predicted unit rows on the device (one 1-D tensor per utterance), ref_units [B, T] the
    de-duplicated reference units -> [(errors, n_ref, n_hyp)] per utterance: the distance between the REDUCED prediction and the
    reference, one reduction launch, one distance launch and one copy back for the batch."""
    B, T = len(pred), max([int(p.shape[0]) for p in pred] + [1])
    dev = ref_units.device
    hyp = torch.zeros(B, T, dtype=torch.int32, device=dev)
    for j, p in enumerate(pred):
        hyp[j, : p.shape[0]] = p
    plen = torch.tensor([int(p.shape[0]) for p in pred], dtype=torch.int32).to(dev)
    red, rlen, _, _ = reduce_units(hyp, plen)
    ref_len = ref_len.to(dev, torch.int32)
    er = _error_rate(edit_distance(red, ref_units, rlen, ref_len), rlen, ref_len)
    return list(zip(er.errors, er.ref_len, er.hyp_len))
