#!/usr/bin/env python3
"""tests/golden/vocoder.npz: the REAL reference classes -- hifigan.Generator, codehifigan.CodeGenerator, fastspeech2.VariancePredictor
and vocoder.CodeHiFiGANVocoder.forward -- on the tiny configuration and formula-based weights of tests/vocoder_ref.py, in float64
and in float32 on the CPU.  The four reference files are loaded by path; what they import from the rest of fairseq (registries,
datasets, attention modules: nothing the vocoder's forward touches) is replaced by the stubs below.  The weights are loaded in
weight-norm form and folded by the reference's own remove_weight_norm.
Stored: the codes, the durations, the float64 waveforms with and without duration prediction, and the reference's own
float32-vs-float64 max-abs error per utterance.  Before writing: every exp(logd) - 1 is at least 1e-3 from a rounding boundary, the
durations span 1 .. >= 4 with at least one clamped up to 1, and the pre-tanh signal is O(1).
Run where the reference tree is present: python tools/gen_golden_vocoder.py [reference root]"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vocoder_ref as R  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    return m


class _Dropout(nn.Module):  # FairseqDropout: identity in eval mode
    def __init__(self, p, module_name=None):
        super().__init__()
        self.p = p

    def forward(self, x, inplace=False):
        return nn.functional.dropout(x, self.p, self.training)


def load_reference(ref_root):
    """-> (CodeGenerator, CodeHiFiGANVocoder) of the reference tree."""
    sys.dont_write_bytecode = True  # the reference tree may be read-only
    deco = lambda *a, **k: (lambda f: f)
    unused = type("Unused", (), {})
    for name in ("fairseq", "fairseq.data", "fairseq.data.audio", "fairseq.models", "fairseq.models.text_to_speech"):
        _stub(name)
    _stub("fairseq.utils")
    _stub("fairseq.data.data_utils", lengths_to_padding_mask=None)
    _stub("fairseq.data.audio.audio_utils", get_window=None, get_fourier_basis=None, get_mel_filters=None, TTSSpectrogram=unused)
    _stub("fairseq.data.audio.speech_to_text_dataset", S2TDataConfig=unused)
    sys.modules["fairseq.models"].__dict__.update(FairseqEncoder=nn.Module, FairseqEncoderModel=nn.Module, register_model=deco,
                                                  register_model_architecture=deco)
    _stub("fairseq.models.text_to_speech.hub_interface", TTSHubInterface=unused)
    _stub("fairseq.models.text_to_speech.tacotron2", Postnet=unused)
    _stub("fairseq.modules", FairseqDropout=_Dropout, LayerNorm=nn.LayerNorm, MultiheadAttention=unused, PositionalEmbedding=unused)
    mods = {}
    for leaf in ("hifigan", "fastspeech2", "codehifigan", "vocoder"):
        name = "fairseq.models.text_to_speech." + leaf
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, "fairseq", "models", "text_to_speech", leaf + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods["codehifigan"].CodeGenerator, mods["vocoder"].CodeHiFiGANVocoder


def reference_vocoder(CodeGenerator, Vocoder, sd, cfg, dtype):
    """What CodeHiFiGANVocoder.__init__ does after torch.load, in `dtype`: load the weight-norm state dict, eval, fold."""
    model = CodeGenerator(cfg).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    model.eval()
    model.remove_weight_norm()
    voc = Vocoder.__new__(Vocoder)
    nn.Module.__init__(voc)
    voc.model = model
    return voc


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DIFFNORM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    CodeGenerator, Vocoder = load_reference(ref_root)
    cfg, sd = R.TINY_CFG, R.make_state_dict(R.TINY_CFG, R.TINY_SEED)
    v64 = reference_vocoder(CodeGenerator, Vocoder, sd, cfg, torch.float64)
    v32 = reference_vocoder(CodeGenerator, Vocoder, sd, cfg, torch.float32)
    folded = R.fold(sd)
    out = {"n_utts": len(R.TINY_UNITS), "seed": R.TINY_SEED}
    pre_all, all_dur = [], []
    with torch.no_grad():
        for i, units in enumerate(R.TINY_UNITS):
            code = torch.tensor(units)
            out[f"code{i}"] = code.numpy().astype(np.int32)
            valid = code[code >= 0]
            logd = v64.model.dur_predictor(v64.model.dict(valid[None]))[0]
            raw = torch.exp(logd) - 1
            margin = (raw - torch.floor(raw) - 0.5).abs().min().item()
            assert margin >= 1e-3, f"utterance {i}: exp(logd) - 1 within {margin:.2e} of a rounding boundary: choose another TINY_SEED"
            dur = torch.clamp(torch.round(raw).long(), min=1)
            all_dur.append((dur, raw))
            out[f"dur{i}"] = dur.numpy().astype(np.int32)
            for tag, dp in (("dur", True), ("nodur", False)):
                w64 = v64({"code": code.clone()}, dur_prediction=dp).reshape(-1)
                w32 = v32({"code": code.clone()}, dur_prediction=dp).reshape(-1)
                assert w64.numel() == w32.numel() == (int(dur.sum()) if dp else valid.numel()) * int(np.prod(cfg["upsample_rates"]))
                out[f"wav_{tag}{i}"] = w64.numpy()
                out[f"e_ref32_{tag}{i}"] = np.float64((w32.double() - w64).abs().max().item())
                mine, mine_dur = R.vocode(sd, cfg, code, dp, folded=folded)
                assert (mine - w64).abs().max().item() < 1e-9 and (not dp or torch.equal(mine_dur, dur)), "tests/vocoder_ref.py disagrees with the reference"
                print(f"utterance {i} {tag}: {w64.numel()} samples, e_ref32 {out[f'e_ref32_{tag}{i}']:.3e}, rounding margin {margin:.3e}, durations {dur.tolist()}")
            pre_all.append(R.vocode(sd, cfg, code, True, folded=folded, return_pre_tanh=True)[0])
    durs = torch.cat([d for d, _ in all_dur])
    raws = torch.cat([r for _, r in all_dur])
    assert durs.min() == 1 and durs.max() >= 4 and bool((torch.round(raws) < 1).any()), "durations must span 1 .. >= 4 with one clamped up to 1"
    pre = torch.cat(pre_all)
    rms, big = pre.pow(2).mean().sqrt().item(), (pre.abs() > 3).double().mean().item()
    print(f"pre-tanh RMS {rms:.3f}, |.| > 3: {100 * big:.2f} %")
    assert 0.3 <= rms <= 1.5 and big < 0.02, "the generated weights leave the O(1) regime"
    path = os.path.join(ROOT, "tests", "golden", "vocoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
