"""Plain-torch restatement of the CodeHiFiGAN unit vocoder, written from its definition (fairseq/models/text_to_speech/hifigan.py,
codehifigan.py, vocoder.py:214-235, fastspeech2.py:117-151), and the formula-based weights the golden file, the tests and the
benchmark share.  Functional and dtype-generic: float64 is the yardstick, float32 the reference's own arithmetic.

`operand_dtype=torch.float16` is the rounding-points model of the f16 engine: every conv's operands -- the activations after their
`pre` non-linearity and the weights -- are rounded to half, everything else (products, sums, biases, residuals, the duration
predictor) stays in `dtype`.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

TINY_CFG = {
    "embedding_dim": 32, "model_in_dim": 32, "num_embeddings": 60, "upsample_initial_channel": 128,
    "upsample_rates": [5, 4, 2], "upsample_kernel_sizes": [11, 8, 4],
    "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
    "dur_predictor_params": {"encoder_embed_dim": 32, "var_pred_hidden_dim": 32, "var_pred_kernel_size": 3, "var_pred_dropout": 0.5},
}
FULL_CFG = {
    "embedding_dim": 128, "model_in_dim": 128, "num_embeddings": 1000, "upsample_initial_channel": 512,
    "upsample_rates": [5, 4, 4, 2, 2], "upsample_kernel_sizes": [11, 8, 8, 4, 4],
    "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
    "dur_predictor_params": {"encoder_embed_dim": 128, "var_pred_hidden_dim": 128, "var_pred_kernel_size": 3, "var_pred_dropout": 0.5},
}
# the edge tests' configuration: every wave arrangement of the conv operator (C_out 128 ... 16 and 1) at a size where float64 on
# the CPU stays under a second for an utterance of 300 units
EDGE_CFG = {
    "embedding_dim": 32, "model_in_dim": 32, "num_embeddings": 60, "upsample_initial_channel": 128,
    "upsample_rates": [4, 2, 2], "upsample_kernel_sizes": [8, 4, 4],
    "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]],
    "dur_predictor_params": {"encoder_embed_dim": 32, "var_pred_hidden_dim": 32, "var_pred_kernel_size": 3, "var_pred_dropout": 0.5},
}
TINY_SEED, FULL_SEED = 3, 11


def predictor_cfg(hidden: int) -> dict:
    """The smallest generator the engine accepts (no activation wider than 32 floats per unit) under a duration predictor of the
    given hidden width: for tests that run the predictor alone."""
    return {
        "embedding_dim": 32, "model_in_dim": 32, "num_embeddings": 60, "upsample_initial_channel": 32,
        "upsample_rates": [2], "upsample_kernel_sizes": [4], "resblock_kernel_sizes": [3], "resblock_dilation_sizes": [[1, 3, 5]],
        "dur_predictor_params": {"encoder_embed_dim": 32, "var_pred_hidden_dim": hidden, "var_pred_kernel_size": 3, "var_pred_dropout": 0.5},
    }
# the golden file's utterances: 13, 1, 7 and 12 units (one -1 among the 14 codes of the first)
TINY_UNITS = [[7, 41, 41, 3, -1, 58, 12, 12, 29, 0, 33, 17, 59, 21], [26], [5, 5, 48, 19, 36, 2, 50], [44, 9, 31, 31, 14, 55, 23, 6, 38, 1, 47, 20]]


# ------------------------------------------------------------------------------------------------ weights by formula
def _unit(n: int, key: int) -> torch.Tensor:
    """n values of unit variance, uniform in (-sqrt 3, sqrt 3), from a splitmix64 hash of (key, index): the same on every platform."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(key) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return torch.from_numpy((2.0 * u - 1.0) * math.sqrt(3.0))


def make_state_dict(cfg: dict, seed: int, weight_norm: bool = True, proj_scale: float = 1.0, proj_bias: float = 0.85) -> dict:
    """Float64 generator state dict under the reference's parameter names.  Not init_weights' std 0.01 (every signal would vanish):
    each conv keeps its input's scale (gain over fan-in, leaky ReLU's loss made up), the second conv of a ResBlock pair is a quarter
    of that so the residual stream stays O(1) through three pairs, and conv_post lands the pre-tanh signal at RMS ~ 0.7.
    `proj_scale` multiplies the duration predictor's proj.weight (0: every log duration is exactly `proj_bias`), `proj_bias` is its
    bias; the defaults are the fixtures' values."""
    sd, key = {}, [seed * 1000]

    def rnd(*shape, std=1.0):
        key[0] += 1
        return (_unit(int(np.prod(shape)), key[0]) * std).reshape(*shape)

    def conv(name, c_out, c_in, k, gain, transposed=False, stride=1):
        fan = c_in * k / stride
        w = rnd(c_in, c_out, k, std=gain / math.sqrt(fan)) if transposed else rnd(c_out, c_in, k, std=gain / math.sqrt(fan))
        if weight_norm:  # g is not the norm of v: the fold has something to do
            scale = 0.5 + rnd(w.shape[0], 1, 1).abs()
            sd[name + ".weight_v"] = w * scale
            sd[name + ".weight_g"] = w.norm(2, dim=(1, 2), keepdim=True)
        else:
            sd[name + ".weight"] = w
        sd[name + ".bias"] = rnd(c_out, std=0.05)

    E, C = cfg["embedding_dim"], cfg["upsample_initial_channel"]
    sd["dict.weight"] = rnd(cfg["num_embeddings"], E)
    conv("conv_pre", C, E, 7, 1.0)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        conv(f"ups.{i}", C // 2, C, k, 1.35, transposed=True, stride=u)
        C //= 2
        for j, rk in enumerate(cfg["resblock_kernel_sizes"]):
            for m in range(3):
                conv(f"resblocks.{i * nk + j}.convs1.{m}", C, C, rk, 1.35)
                conv(f"resblocks.{i * nk + j}.convs2.{m}", C, C, rk, 0.35)
    conv("conv_post", 1, C, 7, 0.9)
    dp = cfg.get("dur_predictor_params")
    if dp:
        H, p = dp["var_pred_hidden_dim"], "dur_predictor."
        for name, c_in in (("conv1.0", E), ("conv2.0", H)):
            sd[p + name + ".weight"] = rnd(H, c_in, 3, std=1.4 / math.sqrt(3 * c_in))
            sd[p + name + ".bias"] = rnd(H, std=0.05)
        for ln in ("ln1", "ln2"):
            sd[p + ln + ".weight"] = 1.0 + rnd(H, std=0.1)
            sd[p + ln + ".bias"] = rnd(H, std=0.05)
        sd[p + "proj.weight"] = rnd(1, H, std=0.75 / math.sqrt(H)) * proj_scale
        sd[p + "proj.bias"] = torch.full((1,), proj_bias, dtype=torch.float64)
    return sd


def fold(sd: dict, dtype=torch.float64) -> dict:
    """remove_weight_norm on a state dict: weight = v * g / ||v||, the norm over every axis but the first (weight_norm's dim = 0:
    the out-channel of a Conv1d, the in-channel of a ConvTranspose1d)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            continue
        if k.endswith(".weight_v"):
            g, vv = sd[k[:-2] + "_g"].to(dtype), v.to(dtype)
            out[k[:-9] + ".weight"] = vv * (g / vv.norm(2, dim=(1, 2), keepdim=True))
        else:
            out[k] = v.to(dtype)
    return out


# ------------------------------------------------------------------------------------------------ the model
def _rnd(t, operand_dtype):
    return t if operand_dtype is None else t.to(operand_dtype).to(t.dtype)


def _conv(x, w, b, dilation=1, operand_dtype=None):
    k = w.shape[2]
    return F.conv1d(_rnd(x, operand_dtype), _rnd(w, operand_dtype), None, padding=(k - 1) // 2 * dilation, dilation=dilation) + b[None, :, None]


def log_durations(sd, cfg, x):
    """VariancePredictor (fastspeech2.py:117-151) on x [1, T, E], eval mode -> log durations [T]."""
    p = "dur_predictor."
    H = cfg["dur_predictor_params"]["var_pred_hidden_dim"]
    h = x
    for conv, ln in (("conv1.0", "ln1"), ("conv2.0", "ln2")):
        h = F.relu(F.conv1d(h.transpose(1, 2), sd[p + conv + ".weight"], sd[p + conv + ".bias"], padding=1)).transpose(1, 2)
        h = F.layer_norm(h, (H,), sd[p + ln + ".weight"], sd[p + ln + ".bias"], 1e-5)
    return F.linear(h, sd[p + "proj.weight"], sd[p + "proj.bias"]).reshape(-1)


def durations_from_log(logd):
    return torch.clamp(torch.round(torch.exp(logd) - 1).long(), min=1)


def generator(sd, cfg, x, operand_dtype=None, return_pre_tanh=False):
    """hifigan.Generator.forward on x [1, C_in, L] with a folded state dict."""
    od = operand_dtype
    x = _conv(x, sd["conv_pre.weight"], sd["conv_pre.bias"], operand_dtype=od)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(_rnd(x, od), _rnd(sd[f"ups.{i}.weight"], od), None, stride=u, padding=(k - u) // 2) + sd[f"ups.{i}.bias"][None, :, None]
        xs = None
        for j in range(nk):
            h = x
            for m, d in enumerate(cfg["resblock_dilation_sizes"][j]):
                r = f"resblocks.{i * nk + j}."
                t = _conv(F.leaky_relu(h, 0.1), sd[r + f"convs1.{m}.weight"], sd[r + f"convs1.{m}.bias"], d, od)
                h = _conv(F.leaky_relu(t, 0.1), sd[r + f"convs2.{m}.weight"], sd[r + f"convs2.{m}.bias"], 1, od) + h
            xs = h if xs is None else xs + h
        x = xs / nk
    pre = _conv(F.leaky_relu(x), sd["conv_post.weight"], sd["conv_post.bias"], operand_dtype=od)  # default slope 0.01
    return pre if return_pre_tanh else torch.tanh(pre)


def vocode(sd, cfg, code, dur_prediction, dtype=torch.float64, operand_dtype=None, device="cpu", folded=None, return_pre_tanh=False, durations=None,
           max_frames=None):
    """CodeHiFiGANVocoder.forward on one utterance -> (waveform [n], durations [T] or None).  `sd` in either form; `folded` a
    cached fold(sd, dtype) on `device`.  The duration predictor never rounds its operands; `durations` overrides it (an entry of 0
    drops its unit).  `max_frames` keeps the first so many frames of the generator's input: the engine's frames = min(total, Lmax0)."""
    if folded is None:
        folded = {k: v.to(device) for k, v in fold(sd, dtype).items()}
    code = torch.as_tensor(code).reshape(-1).long()
    code = code[code >= 0].to(device)
    x = folded["dict.weight"][code][None]  # [1, T, E]
    dur = None
    if dur_prediction:
        dur = durations_from_log(log_durations(folded, cfg, x)) if durations is None else torch.as_tensor(durations).to(device).long()
        x = torch.repeat_interleave(x, dur, dim=1)
    if max_frames is not None:
        x = x[:, :max_frames]
    y = generator(folded, cfg, x.transpose(1, 2), operand_dtype, return_pre_tanh)
    return y.reshape(-1), dur
