#!/usr/bin/env python3
"""tests/golden/conformer_encoder.npz: the REAL reference classes -- S2TConformerEncoder (and S2SConformerEncoder over it when its file
loads), ConformerEncoderLayer, RelPositionMultiHeadedAttention, RelPositionalEncoding -- on the tiny configuration and seeded weights
of tests/conformer_ref.py, in float64 and float32 on the CPU.  The reference files are loaded by path under their real dotted names
(oracle/ref_loader.py's stubs around them); S2TConformerEncoder is compiled from its class statement alone, as ref_loader does for the
transformer encoder (the module around it imports the model registry).  load_state_dict(strict=True) pins the key names.
Stored (arrays only): the ragged batch's lengths, the encoder output in float64 and float32, the padding mask, the subsampled lengths,
the reference's own float32-vs-float64 max error, the shortest utterance run ALONE with the max difference to its rows in the batch
(asserted far above fp32 noise: the convolution module is not masked, so the output depends on the padding), and the hypotheses of the
research IterativeRefinementGenerator (max_iter 4, beam 1, adaptive) with this encoder in front of the fixture decoder.
Run where the reference tree is present: python tools/gen_golden_conformer.py"""
import ast
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import conformer_ref as R  # noqa: E402
import ref_loader  # noqa: E402
from gen_golden_nar import build_reference_model  # noqa: E402

SEED_FEATS = 905  # (902-904: a hypothesis hinges on a near-tie, see NOISE)
NOISE = 1e-3  # the engine's fp32 / bf16x3 bar on the encoder output: the stored hypotheses must not hinge on less
LENGTHS = (61, 40, 23, 9)


def load_conformer(Rn):
    """-> (S2TConformerEncoder, S2SConformerEncoder or None) of the reference tree, over its real layer / attention / position classes."""
    mods = sys.modules["fairseq.modules"]
    ref_loader._load("fairseq.modules.rotary_positional_embedding", "fairseq/modules/rotary_positional_embedding.py")
    esp = ref_loader._load("fairseq.modules.espnet_multihead_attention", "fairseq/modules/espnet_multihead_attention.py")
    pe = ref_loader._load("fairseq.modules.positional_encoding", "fairseq/modules/positional_encoding.py")
    mods.ESPNETMultiHeadedAttention, mods.RelPositionMultiHeadedAttention = esp.ESPNETMultiHeadedAttention, esp.RelPositionMultiHeadedAttention
    mods.RotaryPositionMultiHeadedAttention, mods.RelPositionalEncoding = esp.RotaryPositionMultiHeadedAttention, pe.RelPositionalEncoding
    layer = ref_loader._load("fairseq.modules.conformer_layer", "fairseq/modules/conformer_layer.py")
    path = os.path.join(ref_loader.REF, "fairseq/models/speech_to_text/s2t_conformer.py")
    cls = next(n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "S2TConformerEncoder")
    conv = sys.modules["fairseq.models.speech_to_text.modules.convolution"]
    ns = {"FairseqEncoder": sys.modules["fairseq.models"].FairseqEncoder, "math": math, "torch": torch, "Conv1dSubsampler": conv.Conv1dSubsampler,
          "Conv2dSubsampler": conv.Conv2dSubsampler, "PositionalEmbedding": mods.PositionalEmbedding, "RelPositionalEncoding": pe.RelPositionalEncoding,
          "ConformerEncoderLayer": layer.ConformerEncoderLayer,
          "S2TTransformerEncoder": sys.modules["fairseq.models.speech_to_text"].S2TTransformerEncoder,  # (reorder_encoder_out is borrowed from it)
          "lengths_to_padding_mask": sys.modules["fairseq.data.data_utils"].lengths_to_padding_mask,
          "__name__": "fairseq.models.speech_to_text.s2t_conformer"}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), path, "exec"), ns)
    s2t = ns["S2TConformerEncoder"]
    s2s = None
    try:  # the research subclass (no speaker embedding: forward is the parent's); its module imports the whole model zoo
        m = types.ModuleType("fairseq.models.speech_to_text.s2t_conformer")
        m.S2TConformerEncoder = s2t
        sys.modules[m.__name__] = m
        sys.modules.setdefault("research", types.ModuleType("research")).__path__ = []
        sys.modules.setdefault("research.TranSpeech", types.ModuleType("research.TranSpeech")).__path__ = []
        sys.modules["research.TranSpeech.nar_transformer"] = Rn.nar
        s2s = ref_loader._load("refnar.nar_conformer", "research/TranSpeech/nar_conformer.py").S2SConformerEncoder
    except Exception as e:  # noqa: BLE001
        print("S2SConformerEncoder did not load (%s: %s); using S2TConformerEncoder, whose forward it inherits" % (type(e).__name__, e))
    return s2t, s2s


def build_encoder(cls, sd, dtype):
    c = R.TINY
    args = types.SimpleNamespace(encoder_freezing_updates=0, dropout=0.0, encoder_embed_dim=c.embed_dim, encoder_ffn_embed_dim=c.ffn_dim,
                                 encoder_layers=c.layers, encoder_attention_heads=c.heads, no_scale_embedding=False, conv_version="s2t_transformer",
                                 input_feat_per_channel=c.input_dim, input_channels=1, conv_channels=c.conv_channels,
                                 conv_kernel_sizes=",".join(str(k) for k in c.kernel_sizes), max_source_positions=6000,
                                 depthwise_conv_kernel_size=c.depthwise_kernel, attn_type="espnet", pos_enc_type="rel_pos", fp16=False,
                                 target_speaker_embed=False)
    enc = cls(args)
    full = dict(sd)
    for k, v in enc.state_dict().items():  # version buffers only: every weight and running statistic is given
        if k not in full:
            assert k.endswith("num_batches_tracked") or k == "version", k
            full[k] = v
    enc.load_state_dict(full, strict=True)
    return enc.to(dtype).eval()


def main():
    Rn = ref_loader.load_reference_nar()
    s2t, s2s = load_conformer(Rn)
    cls = s2s or s2t
    c, sd = R.TINY, R.make_state_dict(R.TINY, R.TINY_SEED)
    e64, e32 = build_encoder(cls, sd, torch.float64), build_encoder(cls, sd, torch.float32)
    B, L = len(LENGTHS), max(LENGTHS)
    feats, lens = R.make_features(B, L, LENGTHS, c.input_dim, SEED_FEATS)
    out = {"lens": lens.numpy(), "seed_feats": SEED_FEATS, "encoder_class": np.array(cls.__name__)}
    with torch.no_grad():
        o64 = e64(feats.double(), lens)
        o32 = e32(feats, lens)
        x64 = o64["encoder_out"][0]  # [S, B, D]
        pad = o64["encoder_padding_mask"][0]
        out.update(encoder_out=x64.numpy(), encoder_out_f32=o32["encoder_out"][0].numpy(), padding_mask=pad.numpy(),
                   out_lens=e64.subsample.get_out_seq_lens_tensor(lens).numpy())
        out["e_ref32"] = np.float64((o32["encoder_out"][0].double() - x64).abs().max().item())
        mine, mlens = R.encode(sd, c, feats, lens, torch.float64)
        d = (mine.transpose(0, 1) - x64).abs().max().item()
        print(f"{cls.__name__}: output {tuple(x64.shape)}, scale {x64.abs().max().item():.3f}, e_ref32 {out['e_ref32']:.3e}, restatement diff {d:.3e}")
        assert d < 1e-9 * x64.abs().max().item() and mlens.tolist() == out["out_lens"].tolist(), "tests/conformer_ref.py disagrees with the reference"
        # the shortest utterance alone: no padding behind it
        i = int(np.argmin(LENGTHS))
        n = LENGTHS[i]
        a64 = e64(feats[i:i + 1, :n].double(), lens[i:i + 1])["encoder_out"][0][:, 0]  # [S_i, D]
        Si = a64.shape[0]
        assert Si == int(out["out_lens"][i])
        diff = (a64 - x64[:Si, i]).abs().max().item()
        out.update(alone_index=i, alone_out=a64.numpy(), alone_vs_batch=np.float64(diff))
        print(f"utterance {i} alone vs in the batch: max diff {diff:.3e}")
        assert diff > 1e3 * max(out["e_ref32"], 1e-6), "the fixture must show the padding dependence of the unmasked convolution module"
        mine1, _ = R.encode(sd, c, feats[i:i + 1, :n], lens[i:i + 1], torch.float64)
        assert (mine1[0] - a64).abs().max().item() < 1e-9 * x64.abs().max().item()
        # generate(): this encoder in front of the fixture decoder, the research generator
        model, dct = build_reference_model(Rn)
        model.encoder = e32
        model.forward_encoder = lambda inputs: e32(*inputs)
        orig_to = torch.Tensor.to

        def to_cpu(self, *a, **k):
            if k.get("device") == "cuda":
                k = dict(k, device="cpu")
            return orig_to(self, *a, **k)

        torch.Tensor.to = to_cpu
        try:
            gen = Rn.gen.IterativeRefinementGenerator(dct, max_iter=4, beam_size=1, adaptive=True)
            hyps = gen.generate([model], {"net_input": {"src_tokens": feats, "src_lengths": lens}})
        finally:
            torch.Tensor.to = orig_to
        # no decision of the stored hypotheses may be a near-tie: they survive encoder outputs perturbed by +-NOISE
        for draw in range(2):
            noise = (torch.rand(x64.shape, generator=torch.Generator().manual_seed(draw)) * 2 - 1) * NOISE

            def noisy(inputs, noise=noise):
                eo = e32(*inputs)
                eo["encoder_out"] = [eo["encoder_out"][0] + noise]
                return eo

            model.forward_encoder = noisy
            torch.Tensor.to = to_cpu
            try:
                again = gen.generate([model], {"net_input": {"src_tokens": feats, "src_lengths": lens}})
            finally:
                torch.Tensor.to = orig_to
            same = all(torch.equal(a[0]["tokens"], b[0]["tokens"]) and int(a[0]["steps"]) == int(b[0]["steps"]) for a, b in zip(hyps, again))
            assert same, f"a hypothesis changes under +-{NOISE} on the encoder output: choose another SEED_FEATS"
        out["gen_n"] = len(hyps)
        for j, h in enumerate(hyps):
            out[f"gen_h{j}_tokens"], out[f"gen_h{j}_scores"], out[f"gen_h{j}_steps"] = h[0]["tokens"].numpy(), h[0]["positional_scores"].numpy(), \
                np.int64(h[0]["steps"])
            print(f"hypothesis {j}: {h[0]['tokens'].numel()} tokens, {int(h[0]['steps'])} steps")
    path = os.path.join(ROOT, "tests", "golden", "conformer_encoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
