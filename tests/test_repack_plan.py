"""CPU check of packing.repack_plan (no GPU: dn_*_train_create / _offsets are host logic): for a training engine's entry table and
offsets, the plan's descriptors -- carried out by the pure-torch packing.repack_emulate on the flat fp32 master buffer -- give
exactly the tensors pack_eps / pack_vae build from the state dict, byte for byte, in the same order, in every arithmetic dtype;
the tensors the plan leaves alone are the parameter-independent ones.  Then the plugin's --hip-sample-dtype reaches the models."""
import ctypes as C
import os
import types

import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE

# GEGLU inner width int(40 * 8 / 3) = 106: pad columns 106..127 and zero rows inside the value / gate interleave; dim = 40 pads K
# 40 -> 64 and rows 40 -> 128; dim * dim_cond_mult = 320 (the engines need a multiple of 64, so 8 instead of the usual 4)
AWKWARD_EPS = O.EpsConfig(dim=40, latent_dim=8, depth=2, heads=4, dim_head=16, wavenet_layers=3, wavenet_stacks=2, dim_cond_mult=8)
DTYPES = ["f32", "bf16", "f16", "bf16x3"]


@pytest.fixture(scope="module")
def lib():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def train_layout(lib, kind, cfg, dtype_code=0):
    """(entries, offsets, n_params) of the training engine of `cfg`, as tools/gen_train_layout.py reads them: no device touched."""
    from diffnorm_amd import _lib, packing

    if kind == "vae":
        mults = packing.vae_mults(cfg.latent_dim)
        c = _lib.VaeConfig(cfg.dim, cfg.z, cfg.depth, cfg.heads, cfg.dim_head, cfg.stacks, cfg.layers, cfg.vocab, len(mults),
                           (C.c_int32 * 4)(*(mults + [0] * (4 - len(mults)))), dtype_code)
        entries = packing.vae_train_entries(cfg.dim, mults, cfg.depth, cfg.heads, cfg.dim_head, cfg.stacks, cfg.layers, cfg.vocab)
        prefix = "dn_vae_train_"
    else:
        c = _lib.EpsConfig(cfg.dim, cfg.latent_dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.wavenet_layers, cfg.wavenet_stacks,
                           cfg.dim_cond_mult, dtype_code, 2048)
        entries = packing.eps_train_entries(cfg)
        prefix = "dn_eps_train_"
    h = C.c_void_p()
    _lib.check(getattr(lib, prefix + "create")(C.byref(c), C.byref(h)), prefix + "create")
    try:
        offs = (C.c_int64 * len(entries))()
        assert _lib.check(getattr(lib, prefix + "offsets")(h, offs, len(entries)), prefix + "offsets") == len(entries)
        return entries, list(offs), int(getattr(lib, prefix + "param_count")(h))
    finally:
        getattr(lib, prefix + "destroy")(h)


def packed(kind, sd, cfg, code):
    from diffnorm_amd import packing

    if kind == "vae":
        return packing.pack_vae(sd, cfg.dim, packing.vae_mults(cfg.latent_dim), cfg.depth, cfg.heads, cfg.dim_head, cfg.stacks, cfg.layers,
                                cfg.vocab, code)
    return packing.pack_eps(sd, cfg, code)


def independent_tensors(kind, code):
    """Indices, in pack_eps / pack_vae's list, of the tensors that do not depend on the parameters."""
    from diffnorm_amd import _lib

    half = code in (_lib.DN_BF16, _lib.DN_F16)
    wave_kb = lambda base: [] if half else [base + 10, base + 11]  # K-blocked copies: placeholders outside the 2-byte modes
    tf_kb = lambda base: [] if half else [base + 12, base + 13, base + 14]
    if kind == "eps":  # 7 head tensors, WaveNet (12), transformer (15: the gammas of adaptive norms are placeholders), 2, the sinusoidal table
        return sorted(wave_kb(7) + [19 + 8, 19 + 9] + tf_kb(19) + [36])
    n_wave = 2 * len({16: [4, 3, 2], 32: [4, 3], 128: [3]}[CHAIN_VAE.latent_dim])
    return sorted(sum((wave_kb(12 * n) for n in range(n_wave)), []) + tf_kb(12 * n_wave))


# Hand-picked weights, written into one row of every case's state dict, that pin "rounding equals torch's" byte-wise: beyond the f16
# range (saturation at +-65504, 65520 being the tie that rounds to inf without the clamp), round-to-nearest-even ties of bf16 (8
# significand bits) and f16 (11), f16 subnormals with their ties, a signed zero, an fp32 subnormal, a value near the top of bf16
SPECIALS = [7e4, -1e5, 65504.0, 65519.99, 65520.0, -65520.0,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,
            3e-6, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 6e-8, -2.0 ** -14,
            -0.0, 1e-40, 3.0e38, 1e-30]
SPECIAL_ROW = {"eps": "final_proj.weight", "vae": "decoder_lm.weight"}  # [out, in >= len(SPECIALS)], row 0


def state_dict_with_specials(kind, cfg):
    sd = (O.make_vae_state_dict if kind == "vae" else O.make_eps_state_dict)(cfg, "repack")
    w = sd[SPECIAL_ROW[kind]] = sd[SPECIAL_ROW[kind]].clone()
    assert w.shape[1] >= len(SPECIALS)
    w[0, :len(SPECIALS)] = torch.tensor(SPECIALS, dtype=torch.float32)
    return sd


CASES = {"chain_eps": ("eps", CHAIN_EPS), "chain_vae": ("vae", CHAIN_VAE), "awkward_eps": ("eps", AWKWARD_EPS)}


@pytest.fixture(scope="module")
def masters(lib):
    """case -> (state dict, entries, offsets, flat master): built once, read by every dtype."""
    from diffnorm_amd import packing

    out = {}
    for name, (kind, cfg) in CASES.items():
        sd = state_dict_with_specials(kind, cfg)
        entries, offsets, n = train_layout(lib, kind, cfg)
        out[name] = (sd, entries, offsets, packing.pack_flat(sd, entries, offsets, n))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_plan_reproduces_the_host_packer(masters, case, dtype):
    from diffnorm_amd import engine, packing

    kind, cfg = CASES[case]
    code = engine._dtype_code(dtype)
    sd, entries, offsets, master = masters[case]
    want = packed(kind, sd, cfg, code)
    plan = packing.repack_plan(entries, offsets, code, kind=kind)
    got = packing.repack_emulate(master, plan, code)
    assert len(got) == len(want) == len(plan.shapes)
    assert [i for i, t in enumerate(got) if t is None] == independent_tensors(kind, code)
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (i, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), f"tensor {i} differs"
    # destination order, and every byte of every planned tensor written exactly once
    assert [it.tensor for it in plan.items] == sorted(it.tensor for it in plan.items)
    written = {}
    for it in plan.items:
        nbytes = it.mats * it.rows * it.K * (4 if it.kind in (2, 3) or code in (0, 2) else 2)
        assert it.dst_byte == written.get(it.tensor, 0), it
        written[it.tensor] = it.dst_byte + nbytes
    for i, s in enumerate(plan.shapes):
        if s is not None:
            assert written[i] == got[i].numel() * got[i].element_size(), i


def test_special_weights_reach_the_saturation_and_tie_paths(masters):
    """The hand-picked row arrives in the plan's output as torch rounds it: saturated, ties to even, subnormals kept."""
    from diffnorm_amd import _lib, packing

    sd, entries, offsets, master = masters["awkward_eps"]
    i = 7 + 12 + 15  # final_W in pack_eps's list
    row = lambda code: packing.repack_emulate(master, packing.repack_plan(entries, offsets, code, kind="eps"), code)[i][0]
    h = row(_lib.DN_F16)[:len(SPECIALS)].float().tolist()
    assert h[:6] == [65504.0, -65504.0, 65504.0, 65504.0, 65504.0, -65504.0]
    assert h[10:14] == [1.0, 1 + 2.0 ** -9, -1.0, 1 + 2.0 ** -10]                  # f16 ties to even; just above a tie rounds up
    assert h[14:20] == [50 * 2.0 ** -24, 2.0 ** -24, 0.0, 2.0 ** -23, 2.0 ** -24, -2.0 ** -14]
    b = row(_lib.DN_BF16)[:len(SPECIALS)].float().tolist()
    assert b[6:10] == [1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7]                    # bf16 ties to even; just above a tie rounds up
    assert b[0] == 70144.0 and b[21] != 0.0 and 2.9e38 < b[22] < 3.1e38  # no saturation in bf16; the fp32 subnormal survives
    x = row(_lib.DN_BF16X3)[:64].float().view(2, 32)                               # [lo | hi] of the row's first 32 elements
    assert torch.equal(x[1][:len(SPECIALS)], row(_lib.DN_BF16)[:len(SPECIALS)].float())
    want_lo = (torch.tensor(SPECIALS) - x[1][:len(SPECIALS)]).to(torch.bfloat16).float()
    assert torch.equal(x[0][:len(SPECIALS)], want_lo) and float(want_lo[6]) == 2.0 ** -8


# ------------------------------------------------------------------------------------------ plugin parsers
def _diffusion_args(**kw):
    return types.SimpleNamespace(arch="diff_discrete", criterion="ddpm_discrete_loss", latent_dim=CHAIN_VAE.latent_dim, feature_dim=CHAIN_VAE.dim,
                                 denoiser_dim=CHAIN_EPS.dim, hip_dtype="bf16", multitask=True, diffusion_timesteps=200, speech_decoder_ckpt=None,
                                 target_code_size=1000, data="", **kw)


def test_plugin_sample_dtype_flag_reaches_the_models():
    import argparse

    from diffnorm_amd import fairseq_plugin  # noqa: F401  (registers the names)
    from diffnorm_amd.fairseq_plugin import registry

    for arch in ("diff_discrete", "speech_vae_decoder"):
        p = argparse.ArgumentParser()
        registry.MODEL_REGISTRY[arch].add_args(p)
        assert p.get_default("hip_dtype") == "bf16"  # unchanged
        act = next(a for a in p._actions if "--hip-sample-dtype" in a.option_strings)
        assert act.default is None and sorted(act.choices) == ["bf16", "bf16x3", "f16", "f32"]
        assert p.parse_args(["--hip-sample-dtype", "f16"]).hip_sample_dtype == "f16"
        assert p.parse_args([]).hip_sample_dtype is None

    vargs = dict(arch="speech_vae_decoder", criterion="speech_vae_decoder_loss", latent_dim=32, feature_dim=192, hip_dtype="bf16",
                 target_code_size=1000, data="")
    task = registry.TASK_REGISTRY["speech_decoder"].setup_task(types.SimpleNamespace(**vargs))
    model = task.build_model(types.SimpleNamespace(**vargs, hip_sample_dtype="f16"))
    assert model.encoder.arith == "bf16" and model.encoder.sample_dtype == "f16"
    before = task.build_model(types.SimpleNamespace(**vargs))  # a namespace without the attribute: exactly as before
    assert before.encoder.arith == "bf16" and before.encoder.sample_dtype is None

    dtask = registry.TASK_REGISTRY["speech_diffusion_discrete"].setup_task(_diffusion_args())
    dm = dtask.build_model(_diffusion_args(hip_sample_dtype="f16"))
    assert dm.encoder.model.arith == "bf16" and dm.encoder.model.sample_dtype == "f16"
    assert dm.encoder.speech_decoder.sample_dtype == "f16"
    dm0 = dtask.build_model(_diffusion_args())
    assert dm0.encoder.model.sample_dtype is None and dm0.encoder.speech_decoder.sample_dtype is None
