"""Multi-GPU sharding of the normalisation path: utterance batches are independent, so ranks take whole batches
round-robin with replicated weights and there is no collective in the data path; the only exchange is the final
gather of the (tiny) unit sequences.  One process per GPU (`torch.distributed`, backend "nccl" = RCCL on ROCm, "gloo"
in the CPU tests)."""
from typing import Any, List, Optional, Sequence

import torch.distributed as dist


def rank_world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def batch_indices(n_items: int, batch_size: int) -> List[range]:
    """The reference's batching: consecutive groups of `batch_size` utterances
    (reference research/TranSpeech/diff_norm_synthesis.py:70-129, batches of 100)."""
    return [range(s, min(s + batch_size, n_items)) for s in range(0, n_items, batch_size)]


def my_batches(n_batches: int, rank: int, world: int) -> List[int]:
    """Batch ids of this rank: round-robin, so every rank keeps the reference's batch composition
    (results are bit-identical to a single-GPU run) and loads differ by at most one batch."""
    return list(range(rank, n_batches, world))


def gather_in_order(local: Sequence[Any], local_ids: Sequence[int], n_total: int, group=None) -> List[Any]:
    """All ranks receive the per-batch results of every rank, ordered by batch id."""
    rank, world = rank_world(group)
    if world == 1:
        out = [None] * n_total
        for i, r in zip(local_ids, local):
            out[i] = r
        return out
    parts = [None] * world
    dist.all_gather_object(parts, (list(local_ids), list(local)), group=group)
    out = [None] * n_total
    for ids, res in parts:
        for i, r in zip(ids, res):
            out[i] = r
    missing = [i for i, r in enumerate(out) if r is None]
    if missing:
        raise RuntimeError(f"batches {missing} were produced by no rank")
    return out


# ------------------------------------------------------------------------------------------ batch-independent normalisation
_M64 = (1 << 64) - 1


def utterance_keys(seed: int, indices: Sequence[int]):
    """One 64-bit noise key per utterance: splitmix64 of (seed + (index + 1) * 0x9E3779B97F4A7C15) mod 2^64 (Steele, Lea & Flood,
    "Fast splittable pseudorandom number generators", OOPSLA'14: the golden-ratio increment, then the mixer with shifts 30 / 27 / 31).
    -> torch.int64 [len(indices)] holding the uint64 bit patterns (what ops.chain_start / ops.randn_keyed take).  A key depends
    on the seed and the utterance's position in the list only, so however batches are formed an utterance keeps its noise."""
    import torch

    out = []
    for i in indices:
        z = (int(seed) + (int(i) + 1) * 0x9E3779B97F4A7C15) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
        out.append(z - (1 << 64) if z >> 63 else z)
    return torch.tensor(out, dtype=torch.int64)


def key_bits(keys) -> List[int]:
    """The uint64 values of an int64 key tensor."""
    return [int(k) & _M64 for k in keys.tolist()]


def plan_batches(lengths: Sequence[int], max_tokens: int, max_sentences: Optional[int] = None, pad_multiple: int = 1) -> List[List[int]]:
    """Length-sorted batches under a frame budget: utterances in the order (-length, index); a batch's padded T is its first
    (longest) length rounded up to `pad_multiple`, and it takes utterances greedily while (count + 1) * T <= max_tokens and
    count < max_sentences.  An utterance longer than max_tokens forms a batch of one.  -> index lists, longest batch first."""
    if max_tokens < 1 or pad_multiple < 1 or (max_sentences is not None and max_sentences < 1):
        raise ValueError("plan_batches: max_tokens, max_sentences and pad_multiple must be positive")
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    batches: List[List[int]] = []
    T = 0
    for i in order:
        cur = batches[-1] if batches else None
        if cur is not None and (len(cur) + 1) * T <= max_tokens and (max_sentences is None or len(cur) < max_sentences):
            cur.append(i)
        else:
            T = padded_length(int(lengths[i]), pad_multiple)
            batches.append([i])
    return batches


def padded_length(length: int, pad_multiple: int = 1) -> int:
    return -(-length // pad_multiple) * pad_multiple


def balanced_batches(costs: Sequence[int], rank: int, world: int) -> List[int]:
    """Batch ids of this rank when batches differ in cost (B * T frame-rows): batches in descending cost (ties by batch id) go to
    the rank with the least load so far, the lowest rank on ties -- so the largest load exceeds the mean by at most one batch.
    Deterministic and computed identically on every rank; ids come back ascending."""
    load = [0] * world
    mine = []
    for b in sorted(range(len(costs)), key=lambda b: (-int(costs[b]), b)):
        r = min(range(world), key=lambda r: (load[r], r))
        load[r] += int(costs[b])
        if r == rank:
            mine.append(b)
    return sorted(mine)
