"""CPU check of diffnorm_amd/packing.py, byte for byte (no GPU, no library): the ordered tensor lists of pack_eps / pack_vae in the
four arithmetic dtypes and the flat fp32 training buffer reproduce tests/golden/packed_digests.npz (shape, dtype, SHA-256 of
every tensor); unpack_flat inverts pack_flat; and the flat buffer's entries, converted with `_arith`, ARE the inference list's
tensors -- what the bf16x3 training engine's split `work` buffer and the module layer's flat master -> inference engine path
rely on.

The table was generated ONCE, by tools/gen_packed_digests.py on the commit before the inference packers and the training
tables were put on one table of packed tensors, so it pins the bytes that refactor had to keep.  Regenerate it only for a change
that is meant to move a packed byte."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/engine.h's order of one WaveNet's and one transformer's tensors in the inference lists, under the flat table's entry
# names; None = derived for inference only (the summed skip bias, the K-blocked copies)
WAVE = ("init_W", "init_b", "conv_W", "conv_b", "res_W", "res_b", "skip_W", None, "final_W", "final_b", None, None)
TF_LAYER = ("qkv_W", "out_W", "ffin_W", "ffin_b", "ffconv_W", "ffconv_b", "ffout_W", "ffout_b", "g1", "g2")  # stacked over the layers
TF_TAIL = ("pred_gamma", "pred_W", None, None, None)
LIST_LEN = {"eps_even": 37, "eps_odd": 37, "eps_prompt": 55, "vae_16": 89, "vae_32": 65, "vae_128": 41, "eps_recipe": 37}


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_packed_digests", os.path.join(ROOT, "tools", "gen_packed_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "packed_digests.npz"))


def test_inference_lists_reproduce_the_digests(gen, golden):
    cases = gen.inference_cases()
    assert len(cases) == 6 * 4 + 1 and sorted(k for k in golden.files if k.startswith("list/")) == sorted("list/" + c[0] for c in cases)
    checked = 0
    for key, name, code in cases:
        want = [str(s) for s in golden["list/" + key]]
        got = [gen.describe(t) for t in gen.pack(name, code)]
        assert len(got) == len(want) == LIST_LEN[name], (key, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (key, i, g, w)
        checked += len(got)
    assert checked == 4 * (37 + 37 + 55 + 89 + 65 + 41) + 37 == 1333


def _flat(gen, name):
    sd, ents = gen.state_dict(name), gen.entries(name)
    offs, total = gen.contiguous_offsets(ents)
    from diffnorm_amd import packing

    return sd, ents, offs, packing.pack_flat(sd, ents, offs, total)


def test_flat_buffers_reproduce_the_digests_and_unpack_inverts_pack(gen, golden):
    from diffnorm_amd import packing

    assert gen.FLAT == ("eps_even", "eps_odd", "vae_16", "vae_32", "vae_128")
    assert sorted(k for k in golden.files if not k.startswith("list/")) == sorted(p + n for n in gen.FLAT for p in ("flat/", "keys/"))
    keys = 0
    for name in gen.FLAT:
        sd, ents, offs, flat = _flat(gen, name)
        assert [gen.describe(flat)] == [str(s) for s in golden["flat/" + name]], name
        back = packing.unpack_flat(flat, ents, offs)
        assert sorted(back) == [str(k) for k in golden["keys/" + name]] == sorted(sd), name
        for k, v in sd.items():  # fp32 packing only pads and permutes: the inverse is exact
            assert back[k].shape == v.shape and torch.equal(back[k], v.float()), (name, k)
        keys += len(sd)
    assert keys == 81 + 81 + 230 + 162 + 94


def _list_names(name, gen):
    """Flat-table entry name (or tuple of per-layer names, or None) of every position of the case's inference list."""
    if name in gen.VAE:
        kw = gen.VAE[name][0]
        from diffnorm_amd import packing

        n = len(packing.vae_mults(kw["latent_dim"]))
        names = []
        for prefix in [f"encoder_wave.{i}." for i in range(n)] + [f"decoder_wave.{i}." for i in range(n)]:
            names += [w and prefix + w for w in WAVE]
        tf, depth = "decoder_tf.", kw["depth"]
        tail = [t and tf + t for t in TF_TAIL] + ["decoder_lm.W", "decoder_lm.b"]
        gammas = TF_LAYER
    else:
        kw = gen.EPS[name][0]
        names = ["w_freq", "tc_W", "tc_b", "cond_W", "cond_b", "init_W", "init_b"] + [w and "wavenet." + w for w in WAVE]
        tf, depth = "transformer.", kw["depth"]
        tail = list(TF_TAIL) + ["final_W", "final_b", None]  # None: the sinusoidal table
        gammas = TF_LAYER[:8] + (None, None)  # adaptive norms: placeholders in the list, no entry in the table
    names += [t and tuple(f"{tf}layers.{l}.{t}" for l in range(depth)) for t in gammas]
    return names + tail


def test_flat_entries_in_the_arithmetic_dtype_are_the_inference_tensors(gen):
    from diffnorm_amd import packing

    shared = 0
    for name in gen.FLAT:
        sd, ents, offs, flat = _flat(gen, name)
        part = {e.name: flat[o: o + int(np.prod(e.shape))].view(e.shape) for e, o in zip(ents, offs)}
        names = _list_names(name, gen)
        used = set()
        for tag, code in gen.DTYPES:
            tensors = gen.pack(name, code)
            assert len(tensors) == len(names) == LIST_LEN[name]
            for i, (t, nm) in enumerate(zip(tensors, names)):
                if nm is None:
                    continue
                p = torch.stack([part[n] for n in nm]) if isinstance(nm, tuple) else part[nm]
                used.update(nm if isinstance(nm, tuple) else (nm,))
                want = p if t.dtype == torch.float32 else packing._arith(p, code)  # biases, gammas, conditioning stay fp32
                assert want.dtype == t.dtype and want.shape == t.shape and torch.equal(want, t), (name, tag, i, nm)
                shared += 1
        # every entry of the table but the per-block skip biases (the list holds their sum) is a tensor of the list
        assert {e.name for e in ents} - used == {e.name for e in ents if e.name.endswith("skip_b")}, name
    assert shared == 4 * (28 + 28 + 68 + 50 + 32)
