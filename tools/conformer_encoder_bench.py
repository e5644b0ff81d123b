"""Times the Conformer speech encoder (ConformerEncoderEngine: dn_conformer_encoder_forward) at the recipe's size -- 12 layers,
D = 512, H = 8, FFN 2048, conv_channels 1024, depthwise kernel 31, generated weights -- on [32, 512, 80] features (S = 128), and
what it stands next to, in three steps:
  encoder     the engine in f16 and bf16x3;  (a) NarEncoderEngine (the transformer speech encoder) at the same shape and dtypes;
              (b) the plain-torch restatement tests/conformer_ref.py on the GPU through torch-ROCm in the same dtype (f16; fp32 for
              bf16x3) -- it materialises the [B, H, S, 2S - 1] positional scores, as the reference does
  attn_short  (c) dn_rel_attention alone against dn_attention alone at B = 32, T = 128, H = 8, d_k = 64, f16 and fp32
  attn_long   the same at B = 8, T = 1500
Protocol (README "how numbers are taken"): every leg warmed up, then three alternating blocks of five samples per leg, a synchronised
host clock around each sample (an encoder call; ten back-to-back launches of an attention kernel, divided by ten); the median in
ms and the spread (max - min) / median.  Each step runs in a fresh child process under its own time limit; after a step that fails or
runs out of time nothing more is started.  Prints one JSON line.

    python tools/conformer_encoder_bench.py [--blocks 3] [--calls 5] [--step-timeout 240]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = ("encoder", "attn_short", "attn_long")


def measure(legs, blocks, calls, per_sample=1):
    """legs: name -> callable.  -> name -> {ms, spread}."""
    import torch

    for fn in legs.values():  # warm-up (allocations, kernel attributes, route selection)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(blocks):
        for name, fn in legs.items():
            for _ in range(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_sample):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / per_sample)
    out = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"ms": round(med, 4), "spread": round((max(ts) - min(ts)) / med, 3)}
    return out


def encoder_step(a):
    import torch

    import conformer_ref as R
    from diffnorm_amd import nar_decoder, synthetic

    dev = torch.device("cuda:0")
    cfg = R.RECIPE2.__class__(**{**vars(R.RECIPE2), "layers": 12})
    sd = R.make_state_dict(cfg, 31)
    B, L = 32, 512
    feats, lens = R.make_features(B, L, (L,) * B, cfg.input_dim, 32)
    feats, lens_dev = feats.to(dev), lens.to(dev)
    tsd = synthetic.random_nar_encoder_state_dict(seed=4)
    legs = {}
    for dt in ("f16", "bf16x3"):
        conf = nar_decoder.ConformerEncoderEngine(sd, dtype=dt, device=dev)
        nar = nar_decoder.NarEncoderEngine(tsd, dtype=dt, device=dev)
        legs["conformer_" + dt] = lambda e=conf: e.forward(feats, lens_dev)
        legs["a_transformer_" + dt] = lambda e=nar: e.forward(feats, lens_dev)
    for name, tdt in (("b_torch_f16", torch.float16), ("b_torch_f32", torch.float32)):
        dsd = {k: v.to(dev, tdt) for k, v in sd.items()}

        def torch_leg(dsd=dsd, tdt=tdt):
            with torch.no_grad():
                return R.encode(dsd, cfg, feats, lens, tdt)

        legs[name] = torch_leg
    out, ol = legs["conformer_f16"]()
    assert out.shape == (B, 128, cfg.embed_dim) and bool(torch.isfinite(out).all())
    return {"shape": [B, L, cfg.input_dim], "frames": 128, "layers": cfg.layers, **measure(legs, a.blocks, a.calls)}


def attention_step(a, B, T):
    import torch

    from diffnorm_amd import _lib

    dev, H, dk = torch.device("cuda:0"), 8, 64
    lib = _lib.load()
    g = torch.Generator().manual_seed(B + T)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    u, v = (0.3 * torch.randn(H, dk, generator=g)).to(dev), (0.3 * torch.randn(H, dk, generator=g)).to(dev)
    legs, keep = {}, []
    for name, tdt, code in (("f16", torch.float16, _lib.DN_F16), ("f32", torch.float32, _lib.DN_F32)):
        qkv = torch.randn(B, T, 3 * H * dk, generator=g).to(dev, tdt)
        pos = torch.randn(2 * T - 1, H * dk, generator=g).to(dev, tdt)
        out = torch.empty(B, T, H * dk, dtype=tdt, device=dev)
        es = qkv.element_size()
        r = _lib.RelAttnParams()
        p = _lib.AttnParams()
        for s in (r, p):
            s.q, s.k, s.v, s.out = qkv.data_ptr(), qkv.data_ptr() + H * dk * es, qkv.data_ptr() + 2 * H * dk * es, out.data_ptr()
            s.ldq = s.ldk = s.ldv = 3 * H * dk
            s.ldo, s.B, s.T, s.heads, s.dim_head, s.dtype, s.lengths, s.scale = H * dk, B, T, H, dk, code, lens.data_ptr(), dk ** -0.5
        r.pos, r.ldp, r.pos_zero_row, r.pos_rows, r.bias_u, r.bias_v = pos.data_ptr(), H * dk, T - 1, 2 * T - 1, u.data_ptr(), v.data_ptr()
        keep += [qkv, pos, out, r, p]
        stream = _lib.current_stream()
        legs["rel_attention_" + name] = lambda r=r: _lib.check(lib.dn_rel_attention(C.byref(r), stream), "dn_rel_attention")
        legs["attention_" + name] = lambda p=p: _lib.check(lib.dn_attention(C.byref(p), stream), "dn_attention")
    return {"B": B, "T": T, "heads": H, "dim_head": dk, **measure(legs, a.blocks, a.calls, per_sample=10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=STEPS, help="run one step in this process (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        res = encoder_step(a) if a.step == "encoder" else attention_step(a, 32, 128) if a.step == "attn_short" else attention_step(a, 8, 1500)
        print(json.dumps(res))
        return 0
    res = {"blocks": a.blocks, "calls": a.calls}
    for step in STEPS:  # a fresh child per step, each under its own limit; this process never opens the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--blocks", str(a.blocks), "--calls", str(a.calls)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res[step] = "ran out of time"
            print(json.dumps(res))
            return 1
        if r.returncode != 0:
            res[step] = "failed (%d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "")
            print(json.dumps(res))
            return 1
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
