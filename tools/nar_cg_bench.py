"""Times one captured iteration of classifier-free-guided mask-predict decoding (research/TranSpeech/nat_gen.py:196-236) at the
refine leg's shape -- NAR S2UT decoder 512 / 2048 / 6 layers / 8 heads / 1004 units, B = 32, T = 256, S = 128, 10 iterations per
call, scale 0.5 -- in f16 and bf16x3, one fresh child process per arithmetic:
  a  the guided iteration (one decoder pass over 2 B rows + dn_cmlm_guided_step), null half folded (option nar_cg_fold = 1)
  b  the same with nar_cg_fold = 0: the null half's encoder attention evaluated literally (its keys / values re-formed by every pass)
  c  what the library offered before: two dn_nar_decoder_forward passes (the second on keys / values of a broadcast e_null, every
     source length S), the combination and the update of nat_gen.py restated in torch, captured the same way
  d  the existing unguided captured iteration (NARS2UTDecoderModel.refine)
Protocol (README "how numbers are taken"): every leg warmed up (its capture), then three alternating blocks of five calls per leg,
a synchronised host clock around each call; the median of the 15 in ms per iteration and the spread (max - min) / median.
Prints one JSON line.

    python tools/nar_cg_bench.py [--dtypes f16 bf16x3] [--scale 0.5] [--iters 10] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a, dtype):
    import torch

    from diffnorm_amd import _lib, nar_decoder, synthetic

    dev = torch.device("cuda:0")
    B, T, S, n, scale = a.batch, a.frames, a.source, a.iters, a.scale
    model = nar_decoder.NARS2UTDecoderModel(synthetic.random_nar_decoder_state_dict(seed=3), dtype=dtype, device=dev)
    eng = model.engine
    g = torch.Generator().manual_seed(5)
    enc = {"encoder_out": [torch.randn(S, B, 512, generator=g).to(dev)], "encoder_padding_mask": [], "encoder_embedding": [], "encoder_states": [],
           "src_tokens": [], "src_lengths": []}
    lengths = torch.full((B,), T - 1, dtype=torch.long, device=dev)
    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream
    ckv, slen = model._prepared(enc)
    unk, pad = model.unk, model.pad

    class Baseline:
        """Leg c: two plain passes, torch combination, torch update with the step on the device; one captured iteration."""

        def __init__(self):
            e_null = eng.tensors[0][0].float()
            self.ckv_null = eng.cross_kv(e_null[None, None, :].expand(B, S, -1).contiguous())
            self.full = torch.full((B,), S, dtype=torch.int32, device=dev)
            self.tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
            self.scores = torch.zeros(B, T, device=dev)
            self.lc, self.ln = (torch.empty(B, T, eng.vocab, device=dev) for _ in range(2))
            self.step = torch.zeros(1, dtype=torch.int32, device=dev)
            self.idx = torch.arange(T, device=dev)[None, :]
            self.graph = None

        def iteration(self):
            eng.forward(self.tokens, ckv, slen, out=self.lc)
            eng.forward(self.tokens, self.ckv_null, self.full, out=self.ln)
            sc, tk = torch.log_softmax(self.lc + scale * (self.lc - self.ln), -1).max(-1)
            masks = self.tokens.eq(unk)
            tok = torch.where(masks, tk.int(), self.tokens)
            sc = torch.where(masks, sc, torch.zeros_like(sc))
            p = 1.0 - (self.step.float() + 1.0) / n  # 0 in the last iteration: nothing is re-masked
            boundary = ((tok.ne(pad).sum(1, keepdim=True).float() - 2) * p).long()
            sk = torch.zeros_like(masks).scatter(1, sc.sort(-1)[1], self.idx < boundary)
            self.tokens.copy_(tok.masked_fill(sk, unk))
            self.scores.copy_(sc.masked_fill(sk, 0.0))
            self.step.add_(1)

        def run(self, tok0):
            self.tokens.copy_(tok0)
            self.step.zero_()
            k = n
            if self.graph is None:
                self.iteration()
                k -= 1
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream())
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(gr, stream=side):
                        self.iteration()
                torch.cuda.current_stream().wait_stream(side)
                self.graph = gr
            for _ in range(k):
                self.graph.replay()
            return self.tokens

    base = Baseline()
    state0 = model.initialize_output_tokens(enc, None, true_length=lengths + 1)
    tok0 = torch.full((B, T), unk, dtype=torch.int32, device=dev)
    tok0[:, -1] = model.eos

    def guided(fold):
        _lib.set_option("nar_cg_fold", fold)
        return model.guided_mask_predict(enc, lengths, n, scale)

    legs = [("a_guided_fold", lambda: guided(1)), ("b_guided_literal", lambda: guided(0)), ("c_two_passes_torch", lambda: base.run(tok0)),
            ("d_unguided", lambda: model.refine(state0._replace(step=0, max_step=n), enc, n).output_tokens)]

    def timed(fn):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    outs = {}
    for name, fn in legs:  # warm-up: the capture
        _, outs[name] = timed(fn)
        outs[name] = outs[name].clone()
    agree = {k: bool(torch.equal(outs["a_guided_fold"].long(), outs[k].long())) for k in ("b_guided_literal", "c_two_passes_torch")}
    walls = {name: [] for name, _ in legs}
    for _ in range(3):
        for name, fn in legs:
            walls[name] += [timed(fn)[0] for _ in range(5)]
    _lib.set_option("nar_cg_fold", None)
    row = {"dtype": dtype, "tokens_equal_to_a": agree}
    for name, w in walls.items():
        row[name] = {"ms_per_iteration": statistics.median(w) / n, "spread": (max(w) - min(w)) / statistics.median(w)}
    ms = lambda k: row[k]["ms_per_iteration"]
    row["a_over_d"], row["a_over_b"], row["a_over_c"] = ms("a_guided_fold") / ms("d_unguided"), ms("a_guided_fold") / ms("b_guided_literal"), \
        ms("a_guided_fold") / ms("c_two_passes_torch")
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["f16", "bf16x3"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--source", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per arithmetic")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    out = {"B": a.batch, "T": a.frames, "S": a.source, "iters": a.iters, "scale": a.scale, "rows": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("batch", "frames", "source", "iters", "scale")]
    for dtype in a.dtypes:  # a fresh process per arithmetic; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--child={dtype}"] + passed, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = {"dtype": dtype, "why": "time limit"}
            break
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            out["failed"] = {"dtype": dtype, "why": f"exit status {r.returncode}"}
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["rows"].append(row)
        print(f"{dtype}: " + "  ".join(f"{k[0]} {row[k]['ms_per_iteration']:.3f} ms ({row[k]['spread']:.1%})" for k in row if k[1:2] == "_" and isinstance(row[k], dict))
              + f"  a/d {row['a_over_d']:.3f}  a/b {row['a_over_b']:.3f}  a/c {row['a_over_c']:.3f}", flush=True)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
