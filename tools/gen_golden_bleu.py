"""Writes tests/golden/bleu_stats.json: the statistics fairseq's own BLEU records for seeded pairs of integer sequences, beside the
pairs themselves -- what tests/test_bleu_host.py pins the Counter restatement (tests/bleu_ref.py) to and tests/test_hip_bleu.py the
device.

The reference's fairseq/clib/libbleu/libbleu.cpp is built with g++ into a temporary directory OUTSIDE the repository and `bleu_add`
is called through ctypes, once per pair on a zeroed statistics block.  Two hazards of that code (libbleu.cpp:28-57): bleu_rtrim
underflows on an empty row, so only non-empty rows are recorded; and both rows are trimmed of pad / eos, so pad = -1 and eos = -2
are passed, values no row holds (ids are >= 0).  A third was found here: its n-gram table is keyed by bleu_hash (libbleu.cpp:59-71), an
FNV-style hash over the tokens' bytes, and that hash COLLIDES on real data -- small ids are mostly zero bytes.  On a seeded pair of
1777 / 2000 tokens over alphabet 1004 the bigrams (214, 312) and (40, 454) share the hash 0x363bd56427bed620 (three more such pairs
in the same rows) and bleu_add reports match2 = 889 where 887 bigrams are shared.  So the restatement is asserted equal on every
pair recorded here -- no recorded number rests on a collision --, and the long pairs are drawn over alphabets 2 and 4, whose few
distinct n-grams do not collide; long rows over alphabet 1004 are held to the restatement alone (tests/test_hip_bleu.py).

Recorded: 300 pairs of lengths 1 .. 70 over alphabets 2, 4 and 1004, half of the hypotheses sharing a prefix with their reference,
and 4 pairs of 1000 .. 2000 tokens (alphabets 2 and 4); each as {"hyp", "ref", "stats"} with stats in the device's order [hyp_len, ref_len, match1,
count1, ..., match4, count4].  "corpus": the column sums of the short pairs, and "scorer_score": Scorer.score() of the reference
(fairseq/scoring/bleu.py:132-151) after Scorer.add of every short pair -- the class is loaded where it lies through
oracle/ref_loader.py's leaf-file loader, with the registry / tokenizer names its file imports stubbed and `fairseq.libbleu`
pointing at the library built above.  Nothing compiled from the reference and none of its text is written to the repository."""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import bleu_ref as R  # noqa: E402
import ref_loader  # noqa: E402

PAD, EOS, UNK = -1, -2, -3
SEED = 20240
N_SHORT = 300
LONG = ((2, 1000, 1500), (4, 2000, 1000), (4, 1777, 2000), (2, 1203, 1203))  # alphabet, hyp_len, ref_len


def draw_pairs():
    rng = np.random.RandomState(SEED)
    pairs = []
    for i in range(N_SHORT):
        alphabet = (2, 4, 1004)[i % 3]
        ref = rng.randint(0, alphabet, size=rng.randint(1, 71))
        hyp = rng.randint(0, alphabet, size=rng.randint(1, 71))
        if i % 2:  # the hypothesis starts as its reference does: matches of every order
            k = rng.randint(1, min(len(hyp), len(ref)) + 1)
            hyp[:k] = ref[:k]
        pairs.append((hyp.tolist(), ref.tolist()))
    for alphabet, nh, nr in LONG:
        ref = rng.randint(0, alphabet, size=nr)
        hyp = rng.randint(0, alphabet, size=nh)
        k = min(nh, nr) // 2
        hyp[:k] = ref[:k]
        pairs.append((hyp.tolist(), ref.tolist()))
    return pairs


def build_libbleu(tmp):
    src = os.path.join(ref_loader.REF, "fairseq/clib/libbleu/libbleu.cpp")
    so = os.path.join(tmp, "libbleu_ref.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    return so


class Stat(ctypes.Structure):  # bleu_stat's ten size_t fields, libbleu.cpp:15-26
    _fields_ = [(n, ctypes.c_size_t) for n in ("reflen", "predlen", "match1", "count1", "match2", "count2", "match3", "count3", "match4", "count4")]


def recorded_stats(lib, hyp, ref):
    st = Stat()
    lib.bleu_zero_init(ctypes.byref(st))
    h, r = (ctypes.c_int * len(hyp))(*hyp), (ctypes.c_int * len(ref))(*ref)
    lib.bleu_add(ctypes.byref(st), ctypes.c_size_t(len(ref)), r, ctypes.c_size_t(len(hyp)), h, ctypes.c_int(PAD), ctypes.c_int(EOS))
    return [st.predlen, st.reflen, st.match1, st.count1, st.match2, st.count2, st.match3, st.count3, st.match4, st.count4]


def reference_scorer(so):
    """The reference's Scorer class, or None with the reason printed."""
    try:
        ref_loader.load_reference_optim()  # leaves the fairseq package stubs and an inert fairseq.dataclass in sys.modules
        scoring = types.ModuleType("fairseq.scoring")
        scoring.__path__ = []
        scoring.BaseScorer = type("BaseScorer", (), {})
        scoring.register_scorer = lambda name, dataclass=None: (lambda cls: cls)
        sys.modules["fairseq.scoring"] = scoring
        tok = types.ModuleType("fairseq.scoring.tokenizer")
        tok.EvaluationTokenizer = type("EvaluationTokenizer", (), {"ALL_TOKENIZER_TYPES": str})
        sys.modules["fairseq.scoring.tokenizer"] = tok
        lb = types.ModuleType("fairseq.libbleu")
        lb.__file__ = so
        sys.modules["fairseq.libbleu"] = lb
        sys.modules["fairseq"].libbleu = lb
        return ref_loader._load("fairseq.scoring.bleu", "fairseq/scoring/bleu.py").Scorer
    except Exception as e:  # noqa: BLE001
        print(f"the reference's Scorer could not be loaded: {type(e).__name__}: {e}")
        return None


def main():
    import torch

    tmp = tempfile.mkdtemp(prefix="bleu_golden_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    try:
        so = build_libbleu(tmp)
        lib = ctypes.CDLL(so)
        lib.bleu_add.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        pairs = draw_pairs()
        rows = []
        for hyp, ref in pairs:
            st = [int(v) for v in recorded_stats(lib, hyp, ref)]
            assert st == R.stats(hyp, ref), (hyp, ref, st, R.stats(hyp, ref))
            rows.append({"hyp": hyp, "ref": ref, "stats": st})
        corpus = R.total([r["stats"] for r in rows[:N_SHORT]])
        out = {"seed": SEED, "pad": PAD, "eos": EOS, "n_short": N_SHORT, "pairs": rows, "corpus": corpus, "scorer_score": None}
        Scorer = reference_scorer(so)
        if Scorer is not None:
            sc = Scorer(types.SimpleNamespace(pad=PAD, eos=EOS, unk=UNK))
            for hyp, ref in pairs[:N_SHORT]:
                sc.add(torch.IntTensor(ref), torch.IntTensor(hyp))
            got = [sc.stat.predlen, sc.stat.reflen, sc.stat.match1, sc.stat.count1, sc.stat.match2, sc.stat.count2, sc.stat.match3,
                   sc.stat.count3, sc.stat.match4, sc.stat.count4]
            assert [int(v) for v in got] == corpus, (got, corpus)
            out["scorer_score"] = sc.score()
            print(f"Scorer.score() over the {N_SHORT} short pairs: {out['scorer_score']!r}; restatement: {R.score(corpus, 'none')!r}")
            print(sc.result_string())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = R.GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(rows)} pairs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
