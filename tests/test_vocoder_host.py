"""CPU checks of the CodeHiFiGAN vocoder's host side: the plain-torch restatement against the golden file of the real reference
classes (tools/gen_golden_vocoder.py), the polyphase repack of the transposed convs, the weight-norm fold, the refusals, and the
fixture's own margins.  No GPU and no reference tree needed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_ref as R
from diffnorm_amd import _lib, vocoder as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocoder.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def tiny():
    sd = R.make_state_dict(R.TINY_CFG, R.TINY_SEED)
    return sd, R.fold(sd)


def test_restatement_reproduces_the_reference(gold, tiny):
    sd, folded = tiny
    assert int(gold["n_utts"]) == len(R.TINY_UNITS) and int(gold["seed"]) == R.TINY_SEED
    for i, units in enumerate(R.TINY_UNITS):
        assert gold[f"code{i}"].tolist() == units
        for tag, dp in (("dur", True), ("nodur", False)):
            wav, dur = R.vocode(sd, R.TINY_CFG, units, dp, folded=folded)
            want = torch.from_numpy(gold[f"wav_{tag}{i}"])
            assert wav.shape == want.shape
            assert (wav - want).abs().max().item() <= 1e-9
            if dp:
                assert dur.tolist() == gold[f"dur{i}"].tolist()


@pytest.mark.parametrize("k,u", list(zip(R.FULL_CFG["upsample_kernel_sizes"], R.FULL_CFG["upsample_rates"])))
def test_polyphase_repack_equals_conv_transpose(k, u):
    g = torch.Generator().manual_seed(k * 16 + u)
    C_in, C_out, L = 6, 5, 9
    w = torch.randn(C_in, C_out, k, generator=g, dtype=torch.float64)
    b = torch.randn(C_out, generator=g, dtype=torch.float64)
    x = torch.randn(1, C_in, L, generator=g, dtype=torch.float64)
    want = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
    assert want.shape[-1] == L * u
    w3, b3 = V.polyphase(w, b, u)
    assert w3.shape == (u * C_out, C_in, 3) and b3.shape == (u * C_out,)
    got = F.conv1d(x, w3, b3, padding=1)                                   # [1, u * C_out, L]
    got = got.reshape(1, u, C_out, L).permute(0, 2, 3, 1).reshape(1, C_out, L * u)  # frame s u + r <- phase r of frame s
    assert (got - want).abs().max().item() <= 1e-12


def test_odd_k_minus_u_is_refused():
    w = torch.zeros(4, 4, 7)
    with pytest.raises(ValueError, match="even"):
        V.polyphase(w, None, 4)
    with pytest.raises(ValueError, match="3 u"):
        V.polyphase(torch.zeros(4, 4, 8), None, 2)
    cfg = dict(R.TINY_CFG, upsample_kernel_sizes=[11, 7, 4])
    with pytest.raises(ValueError, match="even"):
        V.check_config(cfg)


def test_weight_norm_and_folded_forms_pack_identically(tiny):
    """The folded form here comes from torch's own weight_norm / remove_weight_norm on Conv1d and ConvTranspose1d modules (dim = 0:
    out-channel resp. in-channel), in fp32 -- not from the code under test."""
    from torch.nn.utils import remove_weight_norm, weight_norm

    sd, _ = tiny
    cfg = R.TINY_CFG
    folded = {}
    for key, v in sd.items():
        if key.endswith(".weight_g"):
            continue
        if not key.endswith(".weight_v"):
            folded[key] = v.float()
            continue
        name = key[:-9]
        vv, g = v.float(), sd[name + ".weight_g"].float()
        if name.startswith("ups."):
            m = weight_norm(torch.nn.ConvTranspose1d(vv.shape[0], vv.shape[1], vv.shape[2]))
        else:
            m = weight_norm(torch.nn.Conv1d(vv.shape[1], vv.shape[0], vv.shape[2]))
        assert m.weight_g.shape == g.shape, name  # one gain per slice of axis 0
        with torch.no_grad():
            m.weight_v.copy_(vv)
            m.weight_g.copy_(g)
        remove_weight_norm(m)
        folded[name + ".weight"] = m.weight.detach().clone()
    for dtype in ("f32", "f16"):
        a, b = V.pack_vocoder(sd, cfg, dtype), V.pack_vocoder(folded, cfg, dtype)
        assert len(a) == len(b) == 3 + 2 * 3 + 12 * 3 * 3 + 2 + 10
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype and torch.equal(x, y), (dtype, i)
    # a ConvTranspose1d gain along the wrong axis would not even have the stored shape
    assert sd["ups.0.weight_g"].shape == (128, 1, 1) and sd["conv_pre.weight_g"].shape == (128, 1, 1) and sd["ups.1.weight_g"].shape == (64, 1, 1)


def test_packed_conv_weight_layout():
    w = torch.arange(2 * 16 * 3, dtype=torch.float32).reshape(2, 16, 3)
    p32, p16 = V.pack_conv_weight(w, _lib.DN_F32), V.pack_conv_weight(w, _lib.DN_F16)
    assert p32.shape == (16, 48) and p16.shape == (16, 64) and p16.dtype == torch.float16
    assert p32[1, 1 * 16 + 5] == w[1, 5, 1] and p16[1, 2 * 16 + 7] == w[1, 7, 2] and (p16[:, 48:] == 0).all() and (p32[2:] == 0).all()
    wide = torch.randn(3, 256, 3)
    p = V.pack_conv_weight(wide, _lib.DN_F32)  # two passes of 128 channels
    assert p.shape == (16, 2 * 384) and p[2, 384 + 1 * 128 + 9] == wide[2, 128 + 9, 1]
    lib = _lib.load()
    for dt, (ci, co, k) in ((_lib.DN_F32, (256, 3, 3)), (_lib.DN_F16, (16, 2, 3)), (_lib.DN_F16, (512, 1280, 3))):
        assert lib.dn_voc_conv_weight_elems(dt, ci, co, k) == V.pack_conv_weight(torch.zeros(co, ci, k), dt).numel()


def test_refusals(tiny):
    sd, _ = tiny
    cfg = R.TINY_CFG
    for bad in ({"multispkr": True}, {"embedder_params": {"x": 1}}, {"f0": True}, {"model_in_dim": 33},
                {"dur_predictor_params": dict(cfg["dur_predictor_params"], var_pred_kernel_size=5)}):
        with pytest.raises(ValueError):
            V.check_config(dict(cfg, **bad))
        with pytest.raises(ValueError):
            V.CodeHiFiGANVocoder(sd, dict(cfg, **bad))
    for dtype in ("bf16", "bf16x3"):
        with pytest.raises(ValueError, match="significand"):
            V.CodeHiFiGANVocoder(sd, cfg, dtype=dtype)
        with pytest.raises(ValueError, match="significand"):
            V.pack_vocoder(sd, cfg, dtype)
    with pytest.raises(ValueError, match="not supported"):
        V.check_inputs({"code": torch.zeros(1, 3), "f0": torch.zeros(1, 3)})
    with pytest.raises(ValueError):
        V.check_inputs({"spkr": torch.zeros(1)})
    nodur = {k: v for k, v in cfg.items() if k != "dur_predictor_params"}
    with pytest.raises(ValueError, match="dur_predictor_params"):
        V.check_dur_prediction(nodur, True)
    V.check_dur_prediction(nodur, False)
    with pytest.raises(ValueError, match="num_embeddings"):
        V.clean_units(torch.tensor([1, 60]), 60)
    with pytest.raises(ValueError, match="empty"):
        V.clean_units(torch.tensor([-1, -1]), 60)
    with pytest.raises(ValueError, match="empty"):
        V.clean_units(torch.tensor([], dtype=torch.long), 60)
    assert V.clean_units(torch.tensor([[3, -1, 59]]), 60).tolist() == [3, 59]
    # a longer list of kernel sizes is refused for its length, not cut to the rates' (its extra entry is the one that is wrong)
    with pytest.raises(ValueError, match="differ in length"):
        V.check_config(dict(cfg, upsample_kernel_sizes=cfg["upsample_kernel_sizes"] + [5]))
    with pytest.raises(ValueError, match="differ in length"):
        V.check_config(dict(cfg, upsample_rates=cfg["upsample_rates"] + [3]))
    # frame counts read back from the device: a saturated (overflowed) or non-positive sum is refused before buffers are sized
    V.check_frames(torch.tensor([3, 2 ** 31 // 40 - 1], dtype=torch.int32), 40)
    for bad in ([3, 2 ** 31 - 1], [3, 2 ** 31 // 40 + 1], [0, 3], [-5, 3]):
        with pytest.raises(ValueError, match="frames"):
            V.check_frames(torch.tensor(bad, dtype=torch.int32), 40)


def test_c_abi_refusals():
    import ctypes as C

    lib = _lib.load()
    assert lib.dn_voc_conv_tile(_lib.DN_BF16, 16, 16, 3) == -1 and b"significand" in lib.dn_last_error()
    assert lib.dn_voc_conv_tile(_lib.DN_F32, 24, 16, 3) == -1
    assert lib.dn_voc_conv_tile(_lib.DN_F32, 16, 16, 4) == -1
    assert lib.dn_voc_conv_tile(_lib.DN_F16, 16, 1, 11) > 0
    assert lib.dn_voc_conv(None, None) == -1
    p = _lib.VocConvParams()
    assert lib.dn_voc_conv(C.byref(p), None) == -1 and b"dn_voc_conv" in lib.dn_last_error()
    cfg = V.voc_config(R.TINY_CFG, _lib.DN_BF16)
    h = C.c_void_p()
    table = (C.c_void_p * 1)()
    assert lib.dn_voc_create(C.byref(cfg), table, 1, C.byref(h)) == -1 and b"bf16" in lib.dn_last_error()
    cfg = V.voc_config(R.TINY_CFG, _lib.DN_F32)
    assert lib.dn_voc_create(C.byref(cfg), table, 1, C.byref(h)) == -1 and b"packed tensors" in lib.dn_last_error()
    assert lib.dn_voc_workspace_bytes(None, 1, 1) == 0


def test_fixture_margins(gold, tiny):
    sd, folded = tiny
    assert os.path.getsize(GOLDEN) < 512 * 1024
    durs, raws, pre = [], [], []
    for i, units in enumerate(R.TINY_UNITS):
        code = torch.tensor(units)
        code = code[code >= 0]
        raw = torch.exp(R.log_durations(folded, R.TINY_CFG, folded["dict.weight"][code][None])) - 1
        assert (raw - torch.floor(raw) - 0.5).abs().min().item() >= 1e-3
        durs += gold[f"dur{i}"].tolist()
        raws.append(raw)
        pre.append(R.vocode(sd, R.TINY_CFG, units, True, folded=folded, return_pre_tanh=True)[0])
        for tag in ("dur", "nodur"):
            assert 0 < float(gold[f"e_ref32_{tag}{i}"]) < 1e-5
    assert [len([c for c in u if c >= 0]) for u in R.TINY_UNITS] == [13, 1, 7, 12] and any(c < 0 for u in R.TINY_UNITS for c in u)
    assert min(durs) == 1 and max(durs) >= 4 and bool((torch.round(torch.cat(raws)) < 1).any())
    pre = torch.cat(pre)
    assert 0.3 <= pre.pow(2).mean().sqrt().item() <= 1.5 and (pre.abs() > 3).double().mean().item() < 0.02
