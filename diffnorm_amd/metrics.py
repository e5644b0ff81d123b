"""Scores of the recipe's results, computed on the device: the unit error rate of normalisation, the word / character error
rate of a vocoder -> ASR loop, and BLEU of the decoded units (unit BLEU) and of the re-transcribed speech (ASR-BLEU).

The error rates are a unit-cost Levenshtein distance over integer sequences (dn_edit_distance of libdiffnorm_hip.so: one wavefront
per pair, csrc/metrics.hip), units after run-length de-duplication (dn_reduce_units, the device form of normalize.reduce_token).
They replace the `editdistance.eval` calls of fairseq's WER scorer (fairseq/scoring/wer.py:50-58) and the per-utterance loop of
diff_norm_synthesis.py:25-46.  Substitution / insertion / deletion counts, alignments and weighted costs are not done here.

BLEU's device part is the per-pair clipped n-gram statistics over integer ids (dn_bleu_stats: one workgroup per pair, one sort of
the n-gram start positions, csrc/bleu.hip), the integers fairseq's libbleu defines (fairseq/clib/libbleu/libbleu.cpp:73-109,138-156)
and a single-reference sacreBLEU sums; the score over their sums is closed-form float64 arithmetic on the host (BleuScore).  It
replaces the sacrebleu.corpus_bleu calls of research/utils/unit_bleu.py:91,106 and research/TranSpeech/asr_bleu/compute_asr_bleu.py:153.
smooth="none" is fairseq's Scorer.score (fairseq/scoring/bleu.py:132-151); smooth="exp" restates sacreBLEU's default smoothing and is
pinned to that statement and to worked cases, NOT to `sacrebleu` (the module is not available to this project).  Not done here:
sacreBLEU's `13a` tokeniser (tokens are str.split(); text normalisation is the caller's, as for `wer` -- for unit strings and CTC
transcripts of letters and apostrophes `13a` changes nothing, for references with punctuation it does), several references per item,
orders above 4, chrF, and a BLEU hook inside normalize().

Everything on the device is integer arithmetic: a result is exact, and depends on the pair alone."""
import math
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


# ------------------------------------------------------------------------------------------ BLEU
BLEU_ORDER = _lib.BLEU_ORDER
SMOOTHINGS = ("exp", "none")


def bleu_stats(hyp, ref, hyp_len=None, ref_len=None, device=None) -> torch.Tensor:
    """BLEU's per-pair statistics of B pairs -> int32 [B, 10] on the device: hyp_len, ref_len, then match_n, count_n for n = 1 .. 4
    with count_n = max(hyp_len - n + 1, 0) and match_n = sum over distinct n-grams of min(count in hyp, count in ref)
    (libbleu.cpp:73-109).  hyp, ref: the input forms of `edit_distance` (device tensors with lengths, host tensors, lists of
    sequences; rows hold at most 8192 tokens; the same host checks, one pinned upload).  Any int32 token values: only equality of
    tokens matters.  One launch, exact, and a row depends on its pair alone."""
    (h, hl, r, rl), device = _sides([("hyp", hyp, hyp_len), ("ref", ref, ref_len)], device)
    B = h.shape[0]
    if r.shape[0] != B:
        raise ValueError(f"bleu_stats: {B} rows of hyp against {r.shape[0]} rows of ref")
    lib = _lib.load()
    stats = torch.empty(B, _lib.BLEU_STATS, dtype=torch.int32, device=device)
    nbytes = lib.dn_bleu_stats_workspace_bytes(B, h.shape[1], r.shape[1])
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.dn_bleu_stats(h.data_ptr(), h.shape[1], hl.data_ptr(), r.data_ptr(), r.shape[1], rl.data_ptr(), B, stats.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 4, _lib.current_stream()), "dn_bleu_stats")
    return stats


def _check_smooth(smooth: str) -> str:
    if smooth not in SMOOTHINGS:
        raise ValueError(f"smooth {smooth!r} ('exp' or 'none')")
    return smooth


def bleu_precisions(matches: Sequence[int], counts: Sequence[int], smooth: str = "exp") -> List[float]:
    """The four n-gram precisions of summed statistics.  "none": m_n / c_n, 0 where c_n = 0 (Scorer.precision, bleu.py:138-147).
    "exp": walk n = 1 .. 4 with k = 1, stop at the first c_n = 0 (the rest stay 0); where m_n = 0, k <- 2k and p_n = 1 / (k c_n)."""
    _check_smooth(smooth)
    if smooth == "none":
        return [m / c if c > 0 else 0.0 for m, c in zip(matches, counts)]
    out, k = [0.0] * len(matches), 1
    for n, (m, c) in enumerate(zip(matches, counts)):
        if c == 0:
            break
        if m == 0:
            k *= 2
            out[n] = 1 / (k * c)
        else:
            out[n] = m / c
    return out


def bleu_brevity(hyp_len: int, ref_len: int, smooth: str = "exp") -> float:
    """min(1, exp(1 - ref_len / hyp_len)) (Scorer.brevity, bleu.py:149-151); 0.0 for an empty hypothesis, where that line divides by
    zero.  Under "exp": 1 if hyp_len >= ref_len, else exp(1 - ref_len / hyp_len) -- the same number."""
    _check_smooth(smooth)
    if hyp_len == 0:
        return 0.0
    if smooth == "none":
        return min(1, math.exp(1 - ref_len / hyp_len))
    return 1.0 if hyp_len >= ref_len else math.exp(1 - ref_len / hyp_len)


def bleu_score(matches: Sequence[int], counts: Sequence[int], hyp_len: int, ref_len: int, smooth: str = "exp") -> float:
    """BLEU (0 - 100) of summed statistics: BP * exp(sum_n ln p_n / 4) * 100, in float64, ln 0 = -inf.
    "none" (Scorer.score, bleu.py:132-136): any m_n = 0 or c_n = 0 gives 0.0.  "exp" (sacreBLEU's default rule, restated): 0.0 if
    m_1 = 0; zero matches of a higher order are smoothed (bleu_precisions), an order the hypothesis is too short for (c_n = 0) keeps
    p_n = 0, so a hypothesis of fewer than 4 tokens scores 0.0.  An empty hypothesis gives 0.0.  Where no m_n and no c_n is zero
    the two rules are the same number."""
    ps = bleu_precisions(matches, counts, smooth)
    if hyp_len == 0 or matches[0] == 0 or any(p <= 0 for p in ps):
        return 0.0
    psum = sum(math.log(p) for p in ps)
    return bleu_brevity(hyp_len, ref_len, smooth) * math.exp(psum / len(ps)) * 100


@dataclass
class BleuScore:
    """Per-item BLEU statistics: `matches` [B][4] and `totals` [B][4] (the clipped matches and the hypothesis's n-grams of order
    1 .. 4) with the items' hypothesis and reference lengths.  `score` is the corpus BLEU of the SUMMED statistics (not a mean of
    the items), `item_scores` each item scored alone (unit_bleu.py:91); both under `smooth`."""
    matches: List[List[int]]
    totals: List[List[int]]
    hyp_len: List[int]
    ref_len: List[int]
    smooth: str = "exp"

    def __post_init__(self):
        _check_smooth(self.smooth)
        self.matches, self.totals = ([[int(v) for v in row] for row in x] for x in (self.matches, self.totals))
        self.hyp_len, self.ref_len = ([int(v) for v in x] for x in (self.hyp_len, self.ref_len))
        if not len(self.matches) == len(self.totals) == len(self.hyp_len) == len(self.ref_len):
            raise ValueError(f"BleuScore: {len(self.matches)} rows of matches, {len(self.totals)} of totals, {len(self.hyp_len)} hypothesis "
                             f"and {len(self.ref_len)} reference lengths")
        if any(len(row) != BLEU_ORDER for row in self.matches + self.totals):
            raise ValueError(f"BleuScore: every row of matches and totals holds {BLEU_ORDER} orders")

    def __add__(self, other: "BleuScore") -> "BleuScore":
        if not isinstance(other, BleuScore):
            return NotImplemented
        if other.smooth != self.smooth:
            raise ValueError(f"BleuScore: smooth {self.smooth!r} + smooth {other.smooth!r}")
        return BleuScore(self.matches + other.matches, self.totals + other.totals, self.hyp_len + other.hyp_len, self.ref_len + other.ref_len,
                         self.smooth)

    @property
    def total_matches(self) -> List[int]:
        return [sum(row[n] for row in self.matches) for n in range(BLEU_ORDER)]

    @property
    def total_counts(self) -> List[int]:
        return [sum(row[n] for row in self.totals) for n in range(BLEU_ORDER)]

    @property
    def total_hyp_len(self) -> int:
        return sum(self.hyp_len)

    @property
    def total_ref_len(self) -> int:
        return sum(self.ref_len)

    @property
    def precisions(self) -> List[float]:
        return bleu_precisions(self.total_matches, self.total_counts, self.smooth)

    @property
    def brevity_penalty(self) -> float:
        return float(bleu_brevity(self.total_hyp_len, self.total_ref_len, self.smooth))

    @property
    def score(self) -> float:
        return bleu_score(self.total_matches, self.total_counts, self.total_hyp_len, self.total_ref_len, self.smooth)

    @property
    def item_scores(self) -> List[float]:
        return [bleu_score(m, c, h, r, self.smooth) for m, c, h, r in zip(self.matches, self.totals, self.hyp_len, self.ref_len)]

    def format(self) -> str:
        """One line in the shape of Scorer.result_string (bleu.py:153-168)."""
        ratio = self.total_hyp_len / self.total_ref_len if self.total_ref_len else 0.0
        return "BLEU4 = {:2.2f}, {:2.1f}/{:2.1f}/{:2.1f}/{:2.1f} (BP={:.3f}, ratio={:.3f}, syslen={}, reflen={})".format(
            self.score, *[p * 100 for p in self.precisions], self.brevity_penalty, ratio, self.total_hyp_len, self.total_ref_len)


def _bleu_score(stats: torch.Tensor, smooth: str) -> BleuScore:
    rows = stats.cpu().tolist()  # one copy back
    return BleuScore([r[2::2] for r in rows], [r[3::2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], smooth)


def unit_bleu(hyp_units, ref_units, reduce: bool = False, hyp_len=None, ref_len=None, smooth: str = "exp", device=None) -> BleuScore:
    """BLEU between unit sequences (lists of sequences, or padded tensors with hyp_len / ref_len) -> BleuScore; with reduce=True
    after run-length de-duplication of BOTH sides on the device (unit_bleu.py scores the unit strings as they are decoded)."""
    _check_smooth(smooth)
    (h, hl, r, rl), device = _sides([("hyp_units", hyp_units, hyp_len), ("ref_units", ref_units, ref_len)], device)
    if h.shape[0] != r.shape[0]:
        raise ValueError(f"unit_bleu: {h.shape[0]} hypotheses against {r.shape[0]} references")
    if reduce:
        h, hl, _, _ = reduce_units(h, hl)
        r, rl, _, _ = reduce_units(r, rl)
    return _bleu_score(bleu_stats(h, r, hl, rl), smooth)


def bleu(hyps: Sequence[str], refs: Sequence[str], smooth: str = "exp", lowercase: bool = False, device=None) -> BleuScore:
    """Corpus BLEU of `hyps` against one reference each -> BleuScore: the statistics of the str.split() tokens of every pair on the
    device (words -> ids through one dictionary over the batch on the host), the score from their sums.  lowercase: str.lower() of
    both sides first (unit_bleu.py:91,106 pass lowercase=True).  Punctuation and any other text normalisation are left to the caller:
    sacreBLEU's `13a` tokeniser is not applied."""
    _check_smooth(smooth)
    if isinstance(hyps, str) or isinstance(refs, str):
        raise ValueError("bleu: lists of strings are expected, not one string")
    if len(hyps) != len(refs):
        raise ValueError(f"bleu: {len(hyps)} hypotheses against {len(refs)} references")
    if not len(hyps):
        return BleuScore([], [], [], [], smooth)
    if lowercase:
        hyps, refs = [s.lower() for s in hyps], [s.lower() for s in refs]
    h, r = word_ids(hyps, refs)
    return _bleu_score(bleu_stats(h, r, device=device), smooth)
