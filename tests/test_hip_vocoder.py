"""The CodeHiFiGAN vocoder engine on the device: the tiny golden of the real reference classes and the full-size configuration
against the float64 restatement, batch independence bit for bit, workspace regrowth, engine re-creation.

Bars (set by the reference side, never by the engine): f32 -- max-abs error against float64 <= 8 x the reference's own
float32-vs-float64 error (another summation order, the device tanh / exp); f16 -- <= 3 x the error of the rounding-points model
(tests/vocoder_ref.py with operand_dtype=float16) against float64, computed here on the CPU.  Durations are exact in both."""
import os

import numpy as np
import pytest
import torch

import vocoder_ref as R
from diffnorm_amd import vocoder as V

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocoder.npz")
FULL_UNITS = [[5, 900, 33, 17, 256, 731], [12, 640, 77]]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def tiny_sd():
    return R.make_state_dict(R.TINY_CFG, R.TINY_SEED)


@pytest.fixture(scope="module")
def tiny_f16_model(tiny_sd):
    """Error of the f16 rounding-points model against float64, per utterance and duration mode (durations forced to the exact ones)."""
    f32 = R.fold(tiny_sd, torch.float32)
    f64 = R.fold(tiny_sd)
    err = {}
    for i, u in enumerate(R.TINY_UNITS):
        for dp in (True, False):
            w64, dur = R.vocode(tiny_sd, R.TINY_CFG, u, dp, folded=f64)
            w16, _ = R.vocode(tiny_sd, R.TINY_CFG, u, dp, dtype=torch.float32, operand_dtype=torch.float16, folded=f32, durations=dur)
            err[(i, dp)] = (w16.double() - w64).abs().max().item()
    return err


@pytest.fixture(scope="module")
def engines(tiny_sd):
    return {dt: V.CodeHiFiGANVocoder(tiny_sd, R.TINY_CFG, dtype=dt) for dt in ("f32", "f16")}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_tiny_golden(gold, engines, tiny_f16_model, dtype):
    voc = engines[dtype]
    units = [torch.tensor(u) for u in R.TINY_UNITS]
    for tag, dp in (("dur", True), ("nodur", False)):
        wavs = voc.generate(units, dur_prediction=dp)
        for i, wav in enumerate(wavs):
            want = torch.from_numpy(gold[f"wav_{tag}{i}"])
            if dp:
                assert voc.last_durations[i].cpu().tolist() == gold[f"dur{i}"].tolist()
            assert wav.dtype == torch.float32 and wav.dim() == 1 and wav.numel() == want.numel()
            err = (wav.cpu().double() - want).abs().max().item()
            bar = 8 * float(gold[f"e_ref32_{tag}{i}"]) if dtype == "f32" else 3 * tiny_f16_model[(i, dp)]
            print(f"tiny {dtype} {tag} utterance {i}: max abs err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
            assert err <= bar, (dtype, tag, i, err, bar)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_batch_independence_bit_for_bit(engines, dtype):
    voc = engines[dtype]
    units = [torch.tensor(u) for u in R.TINY_UNITS]
    for dp in (True, False):
        base = voc.generate(units, dur_prediction=dp)
        single = [voc.forward({"code": u[None]}, dur_prediction=dp) for u in units]
        perm = [2, 0, 3, 1]
        shuffled = voc.generate([units[i] for i in perm], dur_prediction=dp)
        others = voc.generate([units[1], torch.tensor([3, 3, 9, 40, 41, 42, 0, 1, 2, 59, 58, 57, 30, 31, 32, 33, 34]), units[0], torch.tensor([8])], dur_prediction=dp)
        for i in range(4):
            assert base[i].shape == single[i].shape and torch.equal(base[i], single[i]), (dp, i)
            assert torch.equal(shuffled[perm.index(i)], base[i]), (dp, i)
        assert torch.equal(others[0], base[1]) and torch.equal(others[2], base[0])


@pytest.fixture(scope="module")
def full_ref():
    sd = R.make_state_dict(R.FULL_CFG, R.FULL_SEED)
    f64, f32 = R.fold(sd), R.fold(sd, torch.float32)
    ref = {}
    for i, u in enumerate(FULL_UNITS):
        for dp in (True, False):
            w64, dur = R.vocode(sd, R.FULL_CFG, u, dp, folded=f64)
            w32, dur32 = R.vocode(sd, R.FULL_CFG, u, dp, dtype=torch.float32, folded=f32)
            w16, _ = R.vocode(sd, R.FULL_CFG, u, dp, dtype=torch.float32, operand_dtype=torch.float16, folded=f32, durations=dur)
            assert not dp or torch.equal(dur, dur32)
            ref[(i, dp)] = (w64, dur, (w32.double() - w64).abs().max().item(), (w16.double() - w64).abs().max().item())
    return sd, ref


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_full_size_config(full_ref, dtype):
    sd, ref = full_ref
    voc = V.CodeHiFiGANVocoder(sd, R.FULL_CFG, dtype=dtype)
    assert voc.engine.upsample == 320
    for dp in (True, False):
        wavs = voc.generate([torch.tensor(u) for u in FULL_UNITS], dur_prediction=dp)
        for i, wav in enumerate(wavs):
            w64, dur, e32, e16 = ref[(i, dp)]
            if dp:
                assert voc.last_durations[i].cpu().tolist() == dur.tolist()
            assert wav.numel() == w64.numel() == (int(dur.sum()) if dp else len(FULL_UNITS[i])) * 320
            err = (wav.cpu().double() - w64).abs().max().item()
            bar = 8 * e32 if dtype == "f32" else 3 * e16
            print(f"full {dtype} dur_prediction={dp} utterance {i}: {wav.numel()} samples, max abs err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
            assert err <= bar, (dtype, dp, i, err, bar)


def test_workspace_regrowth_and_recreation(tiny_sd, engines):
    voc = engines["f32"]
    small = voc.generate([torch.tensor([4, 5])], dur_prediction=True)
    big = voc.generate([torch.arange(50) % 60, torch.arange(31) % 60, torch.tensor([4, 5])], dur_prediction=True)
    big_dur = [d.cpu() for d in voc.last_durations]
    again = voc.generate([torch.tensor([4, 5])], dur_prediction=True)
    assert torch.equal(small[0], big[2]) and torch.equal(small[0], again[0])
    for i, n_units in enumerate((50, 31, 2)):
        assert big_dur[i].numel() == n_units
        assert big[i].numel() == int(big_dur[i].sum()) * voc.engine.upsample
    assert torch.isfinite(big[0]).all() and big[0].abs().max() <= 1
    # an engine of its own, used, destroyed (the last reference goes: dn_voc_destroy), and created again
    fresh = V.CodeHiFiGANVocoder(tiny_sd, R.TINY_CFG, dtype="f32")
    one = fresh.generate([torch.tensor([4, 5])], dur_prediction=True)
    assert torch.equal(one[0], small[0])
    handle = fresh.engine.handle
    del fresh
    assert not handle.value, "the engine was not destroyed with its last reference"
    fresh2 = V.CodeHiFiGANVocoder(tiny_sd, R.TINY_CFG, dtype="f32")
    assert torch.equal(fresh2.generate([torch.tensor([4, 5])], dur_prediction=True)[0], small[0])


def test_stage_times_of_a_profiled_forward(engines):
    """set_profile(True), one forward: stage_times() gives n_ups + 2 finite, non-negative ms (embedding + conv_pre, each upsampling stage,
    conv_post); switched off again, the next forward returns the same bits."""
    import math

    voc = engines["f32"]
    units = [torch.tensor(u) for u in R.TINY_UNITS]
    base = voc.generate(units, dur_prediction=True)
    voc.engine.set_profile(True)
    profiled = voc.generate(units, dur_prediction=True)
    times = voc.engine.stage_times()
    voc.engine.set_profile(False)
    assert len(times) == len(R.TINY_CFG["upsample_rates"]) + 2 and all(math.isfinite(t) and t >= 0.0 for t in times), times
    after = voc.generate(units, dur_prediction=True)
    for a, b, c in zip(base, profiled, after):
        assert torch.equal(a, b) and torch.equal(a, c)
