"""Speech-unit normalisation driver: the host-side loop of the reference's
research/TranSpeech/diff_norm_synthesis.py (:25-46 unit de-duplication, :132-171 batch assembly, :200-222 sampling
and TSV lines), sharded over ranks by `diffnorm_amd.sharding`."""
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import sharding

TSV_HEADER = "id\tsrc_audio\tsrc_n_frames\ttgt_audio\ttgt_n_frames"


def reduce_token(tokens: Sequence[int]) -> Tuple[List[int], List[int], torch.Tensor]:
    """Run-length de-duplication: (units without consecutive repeats, run lengths, index of each run's first frame)."""
    dedup, durations, keep = [], [], []
    for i, tok in enumerate(tokens):
        if i == 0 or tok != tokens[i - 1]:
            dedup.append(tok)
            keep.append(i)
            durations.append(1)
        else:
            durations[-1] += 1
    return dedup, durations, torch.tensor(keep, dtype=torch.long)


@dataclass
class Utterance:
    audio_id: str
    src_audio: str
    src_n_frames: int
    feat: object                # [T_full, 768] mHuBERT features of the target speech: a tensor, or the path of its .npy file
    tgt_unit: Sequence[int]     # frame-level units (length T_full)
    reduce_tgt_unit: Sequence[int]  # de-duplicated units

    def features(self) -> torch.Tensor:
        """The feature matrix; a path is read when the utterance's batch is assembled (the reference loads per batch too,
        diff_norm_synthesis.py:132-171), so a rank only ever holds the features of the batch it is working on."""
        if isinstance(self.feat, str):
            import numpy as np

            return torch.from_numpy(np.load(self.feat)).float()
        return self.feat


def assemble_batch(items: Sequence[Utterance], device, pad_to: Optional[int] = None):
    """Selects the first frame of every unit run, zero-pads to the longest utterance (reference :132-171), or to `pad_to` frames
    when given (at least the longest)."""
    feats, units = [], []
    for it in items:
        _, _, keep = reduce_token(list(it.tgt_unit))
        f = it.features()[keep]
        assert f.shape[0] == len(it.reduce_tgt_unit), "reduced units do not match the de-duplicated frames"
        feats.append(f)
        units.append(torch.tensor(list(it.reduce_tgt_unit), dtype=torch.long))
    lens = torch.tensor([f.shape[0] for f in feats], dtype=torch.long)
    B, T = len(items), int(lens.max())
    if pad_to is not None:
        assert pad_to >= T, f"pad_to={pad_to} is shorter than the batch's longest utterance ({T})"
        T = pad_to
    feat = torch.zeros(B, T, feats[0].shape[1])
    unit = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        feat[b, : lens[b]], unit[b, : lens[b]] = feats[b], units[b]
    # one pinned staging buffer + one async copy per tensor instead of one H2D per utterance (reference :145)
    if torch.cuda.is_available():
        feat, unit = feat.pin_memory(), unit.pin_memory()
    return feat.to(device, non_blocking=True), unit.to(device, non_blocking=True), lens.to(device)


def tsv_line(it: Utterance, pred_units: Sequence[int]) -> str:
    dedup, _, _ = reduce_token(list(pred_units))
    return f"{it.audio_id}\t{it.src_audio}\t{it.src_n_frames}\t{' '.join(str(u) for u in dedup)}\t{len(pred_units)}"


def normalize(ddim_sample: Callable, utterances: Sequence[Utterance], start_step: int = 50, batch_size: int = 100,
              device="cuda:0", group=None, sampling_steps: Optional[int] = None, eta: float = 0.0, seed: int = 0,
              solver: Optional[str] = None, noise_seed: Optional[int] = None, max_tokens: Optional[int] = None,
              max_sentences: Optional[int] = None, pad_multiple: int = 1, keyed_steps: bool = False,
              unit_changes: Optional[list] = None) -> Optional[List[str]]:
    """Runs `ddim_sample(feat, input_mask=..., ref_units=..., start_step=...)` (LatentDiscreteModel.ddim_sample) over this
    rank's batches and gathers the TSV lines of all ranks in utterance order (every rank returns the full list).
    `sampling_steps` (evaluations per chain instead of start_step-1), `eta`, `seed` and `solver` ("dpmpp_2m": the second-order
    update for short chains) reach `ddim_sample` only when set.

    `noise_seed`: every utterance draws its posterior and chain-start noise from its own key (sharding.utterance_keys of the seed and
    the utterance's position in `utterances`; passed as `noise_keys=`), on the device, so its result does not depend on the batch
    it is in, on torch's generators or on the number of ranks.  `max_tokens` (needs `noise_seed`): batches are formed by a frame
    budget instead of `batch_size` consecutive utterances -- sharding.plan_batches over the de-duplicated lengths (length-sorted, at
    most `max_sentences` utterances, T rounded up to `pad_multiple`), spread over the ranks by cost (sharding.balanced_batches).
    `pad_multiple` > 1 also rounds the consecutive batches' T up.  `keyed_steps` (needs `noise_seed`): a stochastic chain
    (`eta` != 0) draws its per-step noise from the utterance's key as well (the sampler's `keyed_steps=True`; `seed` is not used),
    so it keeps the same promises; without it `noise_seed` refuses `eta` != 0.  With the five unset this is the reference's batching
    and noise.

    `unit_changes`: a list that receives one `(audio_id, errors, n_ref, n_hyp)` per utterance, in utterance order, on every rank
    (gathered as the lines are): the edit distance between the de-duplicated predicted units and the utterance's `reduce_tgt_unit`
    -- how far normalisation moved the units -- computed on the device from the batch's prediction (metrics.unit_changes) before
    it is brought to the host.  The returned lines do not depend on it."""
    if noise_seed is not None or max_tokens is not None or max_sentences is not None or pad_multiple != 1 or keyed_steps:
        return _normalize_keyed(ddim_sample, utterances, start_step, batch_size, device, group, sampling_steps, eta, solver,
                                noise_seed, max_tokens, max_sentences, pad_multiple, keyed_steps, unit_changes)
    rank, world = sharding.rank_world(group)
    # A run must give the same results on any number of ranks (and whatever sizes the last batches have).  The 2-byte / f32
    # contractions' fast K order (taps of a causal conv innermost, one staged copy of the rows, on the two 256-row tiles) sums in a
    # different order than the small-batch tiles, so by default a large batch and a small one can differ in the last bit of an fp32
    # sum.  normalize() therefore ALWAYS routes the tap contractions by SHAPE, not by batch size (option "taps_inner" = 2: the
    # 256-row tiles and their order at every batch size) -- the same routing on 1 rank and on N, full speed on the 100-utterance
    # batches this driver forms, 256-row tiles on a short last batch -- for the duration of the call, through the library's
    # option entry (dn_set_option; restored on the way out, no environment mutation), unless the caller has chosen a K order
    # (option set, or DN_TAPS_INNER in the environment at start-up; 0 = term-outer everywhere is the other invariant setting,
    # about 6 % per step slower).  The bf16x3 mode is invariant by construction.
    from . import _lib

    chosen = _lib.get_option("taps_inner")
    batches = sharding.batch_indices(len(utterances), batch_size)
    mine = sharding.my_batches(len(batches), rank, world)
    local, changes = [], []
    extra = {}
    if sampling_steps is not None:
        extra["sampling_steps"] = sampling_steps
    if eta != 0.0:
        extra.update(eta=eta, seed=seed)
    if solver is not None:
        extra["solver"] = solver
    with _lib.option("taps_inner", 2 if chosen is None else chosen):
        for b in mine:
            items = [utterances[i] for i in batches[b]]
            feat, ref_units, lens = assemble_batch(items, device)
            mask = torch.arange(feat.shape[1], device=lens.device).view(1, -1) < lens.view(-1, 1)
            pred, _, _, _ = ddim_sample(feat, input_mask=mask, cond_scale=1.0, ref_units=ref_units, start_step=start_step, **extra)
            if unit_changes is not None:
                changes.append(_batch_changes(items, pred, ref_units, lens))
            local.append([tsv_line(it, p.tolist()) for it, p in zip(items, pred)])
    per_batch = sharding.gather_in_order(local, mine, len(batches), group)
    if unit_changes is not None:
        unit_changes.extend(c for got in sharding.gather_in_order(changes, mine, len(batches), group) for c in got)
    return [line for lines in per_batch for line in lines]


def _batch_changes(items, pred, ref_units, lens) -> List[tuple]:
    """(audio_id, errors, n_ref, n_hyp) of a batch, from its prediction while that is still on the device."""
    from . import metrics

    return [(it.audio_id,) + c for it, c in zip(items, metrics.unit_changes(pred, ref_units, lens))]


def _normalize_keyed(ddim_sample, utterances, start_step, batch_size, device, group, sampling_steps, eta, solver, noise_seed,
                     max_tokens, max_sentences, pad_multiple, keyed_steps=False, unit_changes=None) -> List[str]:
    """normalize() with per-utterance noise keys and, under `max_tokens`, frame-budget batches (see normalize)."""
    if noise_seed is None and keyed_steps:
        raise ValueError("normalize: keyed_steps draws the per-step noise from the utterances' keys: set noise_seed")
    if noise_seed is None:
        raise ValueError("normalize: max_tokens / max_sentences / pad_multiple re-form the batches, which changes the results unless "
                         "every utterance has its own noise: set noise_seed")
    if eta != 0.0 and not keyed_steps:
        raise ValueError("normalize: noise_seed alone keys the posterior and chain-start noise; the per-step noise of eta != 0 would "
                         "stay indexed by batch position, so the results would still depend on the batches: set keyed_steps=True to "
                         "draw it from the utterances' keys too")
    if max_tokens is None and max_sentences is not None:
        raise ValueError("normalize: max_sentences caps the batches max_tokens forms; without max_tokens use batch_size")
    from . import _lib

    rank, world = sharding.rank_world(group)
    lengths = [len(u.reduce_tgt_unit) for u in utterances]  # no feature is loaded to plan
    if max_tokens is not None:
        batches = sharding.plan_batches(lengths, max_tokens, max_sentences, pad_multiple)
    else:
        batches = [list(r) for r in sharding.batch_indices(len(utterances), batch_size)]
    padded = [sharding.padded_length(max(lengths[i] for i in ids), pad_multiple) for ids in batches]
    if max_tokens is not None:
        mine = sharding.balanced_batches([len(ids) * T for ids, T in zip(batches, padded)], rank, world)
    else:
        mine = sharding.my_batches(len(batches), rank, world)
    extra = {}
    if sampling_steps is not None:
        extra["sampling_steps"] = sampling_steps
    if solver is not None:
        extra["solver"] = solver
    if eta != 0.0:
        extra["eta"] = eta
    if keyed_steps:
        extra["keyed_steps"] = True
    chosen = _lib.get_option("taps_inner")
    local, changes = [], []
    with _lib.option("taps_inner", 2 if chosen is None else chosen):  # routing by shape, as normalize()
        for b in mine:
            items = [utterances[i] for i in batches[b]]
            feat, ref_units, lens = assemble_batch(items, device, pad_to=padded[b])
            mask = torch.arange(feat.shape[1], device=lens.device).view(1, -1) < lens.view(-1, 1)
            keys = sharding.utterance_keys(noise_seed, batches[b])
            pred, _, _, _ = ddim_sample(feat, input_mask=mask, cond_scale=1.0, ref_units=ref_units, start_step=start_step,
                                        noise_keys=keys, **extra)
            if unit_changes is not None:
                changes.append(_batch_changes(items, pred, ref_units, lens))
            local.append([tsv_line(it, p.tolist()) for it, p in zip(items, pred)])
    per_batch = sharding.gather_in_order(local, mine, len(batches), group)
    lines = [None] * len(utterances)  # back to utterance order
    for ids, got in zip(batches, per_batch):
        for i, line in zip(ids, got):
            lines[i] = line
    if unit_changes is not None:
        ordered = [None] * len(utterances)
        for ids, got in zip(batches, sharding.gather_in_order(changes, mine, len(batches), group)):
            for i, c in zip(ids, got):
                ordered[i] = c
        unit_changes.extend(ordered)
    return lines
