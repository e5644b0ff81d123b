"""The CodeHiFiGAN vocoder engine at its geometry edges: utterances past one 64-lane chunk of the duration scan, the predictor's
LayerNorm / projection at ragged widths, the ends of the duration rule, caller-supplied durations (zeros, the Lmax0 cut, an empty
row, garbage behind a row's length) and the refusals of the C entries.

References are computed here on the CPU in float64 from tests/vocoder_ref.py.  Bars as in test_hip_vocoder.py, set by the reference
side and never by the engine: f32 -- max-abs error against float64 <= 8 x the float32 restatement's own error on the same case;
f16 -- <= 3 x the error of the rounding-points model (operand_dtype=float16).  Durations, frame counts and waveform lengths are exact.

Exact durations need inputs away from rounding ties.  That is a condition on the inputs, asserted at every run (`margins`): every raw
exp(logd) - 1 lies at least 1e-3 from k + 0.5 and the float32 restatement gives the float64 durations.  Seeds chosen for it:
EDGE_SEED = 22 with proj scale 1.0 / bias 1.3 (cases a, b, e), WIDTH_SEED = 19 with bias 1.2 (case c); no utterance is exempt.

The cap at 32 767 frames and NaN -> 1 (case d) are the engine's contract, not the reference's: the reference has no cap and its
round(NaN).long() is undefined.  var_pred_hidden_dim = 144 is outside the engine (a conv's C_in beyond 128 is a multiple of 128), so
that width is pinned as a refusal and 256 stands in for "more than two passes of the 64-lane loops".
Measured on an MI355X: DESIGN 9b."""
import math

import pytest
import torch

import vocoder_ref as R
from diffnorm_amd import _lib
from diffnorm_amd import vocoder as V

pytestmark = pytest.mark.gpu
CFG = R.EDGE_CFG
UP = 16
EDGE_SEED, PROJ_SCALE, PROJ_BIAS = 22, 1.0, 1.3
WIDTH_SEED, WIDTH_BIAS = 19, 1.2
COUNTS = [1, 63, 64, 65, 128, 129, 300]
WIDTHS = [16, 48, 64, 80, 128, 256]
SENTINEL = 7.25          # waveform samples are tanh values: |x| <= 1
DN_EINVAL = -1


def units_of(n, salt):
    return torch.randint(0, CFG["num_embeddings"], (n,), generator=torch.Generator().manual_seed(1000 * salt + n))


def margins(folded64, folded32, cfg, code):
    """Exact float64 durations of one utterance, with the condition that makes them comparable asserted."""
    logd = R.log_durations(folded64, cfg, folded64["dict.weight"][code][None])
    raw = torch.exp(logd) - 1
    gap = (raw - torch.floor(raw) - 0.5).abs().min().item()
    assert gap >= 1e-3, f"an utterance of {code.numel()} units lies {gap:.2e} from a rounding tie: choose another seed"
    dur = R.durations_from_log(logd)
    dur32 = R.durations_from_log(R.log_durations(folded32, cfg, folded32["dict.weight"][code][None]))
    assert torch.equal(dur, dur32), "the float32 restatement disagrees with float64 on a duration: choose another seed"
    return dur


# ------------------------------------------------------------------------------------------------ shared references (computed once)
@pytest.fixture(scope="module")
def edge_sd():
    return R.make_state_dict(CFG, EDGE_SEED, proj_scale=PROJ_SCALE, proj_bias=PROJ_BIAS)


@pytest.fixture(scope="module")
def folds(edge_sd):
    return R.fold(edge_sd), R.fold(edge_sd, torch.float32)


def three_ways(sd, f64, f32, code, dp, durations=None, max_frames=None):
    """-> (float64 waveform, error of the float32 restatement, error of the f16 rounding-points model)."""
    w64, _ = R.vocode(sd, CFG, code, dp, folded=f64, durations=durations, max_frames=max_frames)
    w32, _ = R.vocode(sd, CFG, code, dp, dtype=torch.float32, folded=f32, durations=durations, max_frames=max_frames)
    w16, _ = R.vocode(sd, CFG, code, dp, dtype=torch.float32, operand_dtype=torch.float16, folded=f32, durations=durations, max_frames=max_frames)
    return w64, (w32.double() - w64).abs().max().item(), (w16.double() - w64).abs().max().item()


@pytest.fixture(scope="module")
def long_units():
    return [units_of(n, 1) for n in COUNTS]


@pytest.fixture(scope="module")
def long_ref(edge_sd, folds, long_units):
    f64, f32 = folds
    ref = {}
    for i, u in enumerate(long_units):
        ref[(i, False)] = (None,) + three_ways(edge_sd, f64, f32, u, False)
        dur = margins(f64, f32, CFG, u)
        ref[(i, True)] = (dur,) + three_ways(edge_sd, f64, f32, u, True, durations=dur)
    every = torch.cat([ref[(i, True)][0] for i in range(len(COUNTS))])
    assert int(every.min()) == 1 and int(every.max()) >= 8, "the durations do not spread over 1 ... 8"
    return ref


@pytest.fixture(scope="module")
def engines(edge_sd):
    return {dt: V.CodeHiFiGANVocoder(edge_sd, CFG, dtype=dt) for dt in ("f32", "f16")}


def within_bar(tag, dtype, wav, w64, e32, e16):
    assert wav.dtype == torch.float32 and wav.numel() == w64.numel(), (tag, wav.numel(), w64.numel())
    err = (wav.cpu().double() - w64).abs().max().item()
    bar = 8 * e32 if dtype == "f32" else 3 * e16
    print(f"edges {tag} {dtype}: {wav.numel()} samples, max abs err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
    assert err <= bar, (tag, dtype, err, bar)


# ------------------------------------------------------------------------------------------------ a, b: past one scan chunk
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dp", [False, True], ids=["nodur", "dur"])
def test_past_one_scan_chunk(engines, long_units, long_ref, dp, dtype):
    voc = engines[dtype]
    assert voc.engine.upsample == UP
    wavs = voc.generate(long_units, dur_prediction=dp)
    got_dur = [None if d is None else d.cpu() for d in voc.last_durations]
    for i, n in enumerate(COUNTS):
        dur, w64, e32, e16 = long_ref[(i, dp)]
        if dp:
            assert got_dur[i].tolist() == dur.tolist(), (n, "durations differ from the float64 restatement's")
        assert wavs[i].numel() == (int(dur.sum()) if dp else n) * UP
        within_bar(f"{n} units dur_prediction={dp}", dtype, wavs[i], w64, e32, e16)
        alone = voc.forward({"code": long_units[i][None]}, dur_prediction=dp)
        assert alone.shape == wavs[i].shape and torch.equal(alone, wavs[i]), (n, "the batch differs from the utterance alone")
    others = voc.generate([units_of(200, 2), long_units[-1], units_of(301, 2), units_of(64, 2)], dur_prediction=dp)
    assert torch.equal(others[1], wavs[-1]), "the 300-unit utterance depends on its neighbours"


# ------------------------------------------------------------------------------------------------ c: LayerNorm and projection widths
def predictor_case(H):
    cfg = R.predictor_cfg(H)
    sd = R.make_state_dict(cfg, WIDTH_SEED + H, proj_scale=PROJ_SCALE, proj_bias=WIDTH_BIAS)
    return cfg, sd


@pytest.mark.parametrize("H", WIDTHS)
def test_predictor_widths(H):
    cfg, sd = predictor_case(H)
    f64, f32 = R.fold(sd), R.fold(sd, torch.float32)
    lengths = [70, 1, 33]
    codes = torch.stack([units_of(70, 10 + b) for b in range(3)]).int()
    want = [margins(f64, f32, cfg, codes[b, :n].long()) for b, n in enumerate(lengths)]
    eng = V.CodeHiFiGANEngine(sd, cfg, dtype="f32")
    dur, sums = eng.durations(codes.to(eng.device), torch.tensor(lengths, dtype=torch.int32, device=eng.device))
    dur, sums = dur.cpu(), sums.cpu()
    for b, n in enumerate(lengths):
        assert dur[b, :n].tolist() == want[b].tolist(), (H, b)
        assert int(sums[b]) == int(dur[b, :n].sum()) == int(want[b].sum())
        assert not dur[b, n:].any(), "a duration behind a row's length is not 0"
    print(f"edges predictor width {H}: durations {int(torch.cat(want).min())} ... {int(torch.cat(want).max())} exact")


def test_predictor_width_144_is_refused():
    """C_in of the predictor's second conv: beyond 128 the conv operator takes multiples of 128 only."""
    cfg, sd = predictor_case(144)
    with pytest.raises(ValueError, match="128"):
        V.CodeHiFiGANEngine(sd, cfg, dtype="f32")


# ------------------------------------------------------------------------------------------------ d: the duration rule's ends
B_32766 = math.log(32767.2)  # float64 exp(b) - 1 = 32766.2: 0.3 below the tie at 32766.5


def rule_engine(bias):
    cfg = R.predictor_cfg(32)
    return V.CodeHiFiGANVocoder(R.make_state_dict(cfg, WIDTH_SEED, proj_scale=0.0, proj_bias=bias), cfg, dtype="f32")


@pytest.mark.parametrize("bias,want", [(-5.0, 1), (100.0, 32767), (float("nan"), 1), (B_32766, 32766)], ids=["minus5", "inf", "nan", "32766"])
def test_duration_rule_ends(bias, want):
    if want == 32766:  # the margin of this input, on the bias as the engine holds it (float32)
        b32 = torch.tensor(bias, dtype=torch.float32)
        raw = math.exp(float(b32)) - 1
        assert abs(raw - 32766.2) < 0.05 and abs(raw - math.floor(raw) - 0.5) >= 0.25
        assert int(torch.round(torch.exp(b32) - 1)) == want, "float32 disagrees: no test of the engine"
    elif bias == -5.0:  # round(exp(-5) - 1) = -1: the clamp at 1 decides
        assert int(R.durations_from_log(torch.tensor([bias], dtype=torch.float64))) == want and round(math.exp(bias) - 1) == -1
    elif bias == 100.0:  # inf in float32, beyond the cap in float64
        assert math.isinf(float(torch.exp(torch.tensor(bias, dtype=torch.float32)))) and math.exp(bias) - 1 > want
    eng = rule_engine(bias).engine
    lengths = [70, 5]
    codes = torch.stack([units_of(70, 20), units_of(70, 21)]).int().to(eng.device)
    dur, sums = eng.durations(codes, torch.tensor(lengths, dtype=torch.int32, device=eng.device))
    dur, sums = dur.cpu(), sums.cpu()
    for b, n in enumerate(lengths):
        assert dur[b, :n].tolist() == [want] * n and not dur[b, n:].any()
        assert int(sums[b]) == want * n


def test_saturated_sum_is_refused_before_the_forward():
    voc = rule_engine(100.0)
    eng = voc.engine
    n = 65600  # x 32 767 frames = 2 149 515 200 > 2^31 - 1
    code = units_of(n, 22)
    small = voc.generate([code[:3]], dur_prediction=True)
    assert small[0].numel() == 3 * 32767 * eng.upsample
    dur, sums = eng.durations(code.int()[None].to(eng.device), torch.tensor([n], dtype=torch.int32, device=eng.device))
    assert int(sums[0]) == 2 ** 31 - 1, int(sums[0])
    assert int(dur.min()) == int(dur.max()) == 32767
    before, ws = voc.last_durations, eng._ws
    ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    with pytest.raises(ValueError, match="frames"):
        voc.generate([code], dur_prediction=True)
    assert voc.last_durations is before and len(before) == 1 and before[0].tolist() == [32767] * 3
    assert eng._ws is ws and eng._ws.data_ptr() == ws_ptr and eng._ws.numel() == ws_bytes, "a forward was sized"


# ------------------------------------------------------------------------------------------------ e: caller durations
def c_forward(eng, codes, lengths, durations, Lmax0, ws=None, wav_elems=None):
    """dn_voc_forward on a sentinel-filled waveform and sentinel lengths -> (rc, wav [B, Lmax0 * up], wav_lengths)."""
    B, T = codes.shape
    wav = torch.full((B, Lmax0 * eng.upsample) if wav_elems is None else (B, wav_elems), SENTINEL, dtype=torch.float32, device=eng.device)
    wl = torch.full((B,), -77, dtype=torch.int32, device=eng.device)
    wp, wn = eng._ws_for(B, max(Lmax0, T)) if ws is None else ws
    with torch.cuda.device(eng.device):
        rc = eng.lib.dn_voc_forward(eng.handle, codes.data_ptr(), lengths.data_ptr(), _lib.ptr(durations), B, T, Lmax0, wav.data_ptr(), wl.data_ptr(),
                                    wp, wn, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, wav.cpu(), wl.cpu()


def caller_case():
    """B = 4, Tmax = 70 -> (codes, lengths, durations, Lmax0): row 0 is cut by Lmax0 inside a unit, row 1 has no frames at all,
    row 2 is cut exactly on a unit boundary, row 3 is not cut and has zeros at its head, in the middle, in a run of 3 and at its tail."""
    g = torch.Generator().manual_seed(77)
    T = 70
    lengths = [66, 50, 60, 70]
    dur = torch.zeros(4, T, dtype=torch.long)
    dur[0, :66] = torch.randint(2, 5, (66,), generator=g)
    dur[2, :60] = torch.randint(2, 5, (60,), generator=g)
    dur[3] = torch.randint(1, 3, (70,), generator=g)
    for i in (0, 20, 40, 41, 42, 69):
        dur[3, i] = 0
    dur[0, 7] = 0
    L = int(dur[2, :45].sum())
    cum0 = torch.cumsum(dur[0], 0)
    if bool((cum0 == L).any()):
        dur[0, 0] += 1
    codes = torch.stack([units_of(T, 30 + b) for b in range(4)])
    return codes, lengths, dur, L


@pytest.fixture(scope="module")
def caller_ref(edge_sd, folds):
    f64, f32 = folds
    codes, lengths, dur, L = caller_case()
    cum = [torch.cumsum(dur[b, :n], 0) for b, n in enumerate(lengths)]
    # the case is what its docstring says
    assert int(cum[0][-1]) > L and not bool((cum[0] == L).any()), "row 0 is not cut inside a unit"
    assert int(cum[1][-1]) == 0
    assert int(cum[2][-1]) > L and bool((cum[2] == L).any()), "row 2 is not cut on a unit boundary"
    assert 0 < int(cum[3][-1]) < L, "row 3 is cut"
    assert dur[3, 0] == 0 and dur[3, 20] == 0 and not dur[3, 40:43].any() and dur[3, 69] == 0 and dur[3, 1] > 0 and dur[3, 68] > 0
    ref = {b: three_ways(edge_sd, f64, f32, codes[b, :n], True, durations=dur[b, :n], max_frames=L) for b, n in enumerate(lengths) if b != 1}
    frames = [min(int(c[-1]), L) for c in cum]
    return codes, lengths, dur, L, frames, ref


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_caller_durations(engines, caller_ref, dtype):
    eng = engines[dtype].engine
    codes, lengths, dur, L, frames, ref = caller_ref
    poisoned = codes.clone()
    for b, n in enumerate(lengths):
        poisoned[b, n:] = 10 ** 6 if b % 2 else -7
    dev = lambda t: t.int().contiguous().to(eng.device)
    ln = dev(torch.tensor(lengths))
    rc, wav, wl = c_forward(eng, dev(poisoned), ln, dev(dur), L)
    assert rc == 0
    assert wl.tolist() == [f * UP for f in frames] and wl[1] == 0
    for b in range(4):
        assert (wav[b, frames[b] * UP:] == SENTINEL).all(), (b, "samples behind a row's length were written")
        if b != 1:
            within_bar(f"caller durations row {b} ({frames[b]} of {int(dur[b].sum())} frames)", dtype, wav[b, :frames[b] * UP], *ref[b])
    # what lies in `codes` behind lengths[b] reaches no sample
    rc, clean, wl2 = c_forward(eng, dev(codes), ln, dev(dur), L)
    assert rc == 0 and torch.equal(clean, wav) and torch.equal(wl2, wl)
    # the rows without the empty one: same bits
    keep = [0, 2, 3]
    rc, w3, wl3 = c_forward(eng, dev(codes[keep]), dev(torch.tensor(lengths)[keep]), dev(dur[keep]), L)
    assert rc == 0 and torch.equal(w3, wav[keep]) and torch.equal(wl3, wl[keep])
    # the wrapper: zeros behind a row's length, the same samples
    wv, wlv = eng.forward(dev(poisoned), ln, dev(dur), L)
    assert torch.equal(wlv.cpu(), wl)
    for b in range(4):
        assert torch.equal(wv[b, :frames[b] * UP].cpu(), wav[b, :frames[b] * UP]) and not wv[b, frames[b] * UP:].any()


# ------------------------------------------------------------------------------------------------ f: refusals through the C ABI
def test_c_entry_refusals(engines, edge_sd):
    eng = engines["f32"].engine
    lib = eng.lib
    B, T = 2, 12
    codes = torch.stack([units_of(T, 40), units_of(T, 41)]).int().to(eng.device)
    ln = torch.tensor([12, 5], dtype=torch.int32, device=eng.device)
    dur = torch.full((B, T), 2, dtype=torch.int32, device=eng.device)

    def refused(what, *args, **kw):
        rc, wav, wl = c_forward(eng, *args, **kw)
        assert rc == DN_EINVAL, (what, rc)
        assert what.encode() in lib.dn_last_error(), (what, lib.dn_last_error())
        assert (wav == SENTINEL).all() and (wl == -77).all(), "a refused call wrote"

    ok, _, wl = c_forward(eng, codes, ln, dur, 24)
    assert ok == 0 and wl.tolist() == [24 * UP, 10 * UP]
    refused("without durations", codes, ln, None, T - 1)
    need = int(lib.dn_voc_workspace_bytes(eng.handle, B, 24))
    wp, wn = eng._ws_for(B, 24)
    assert need > 0 and wn >= need + 256
    assert c_forward(eng, codes, ln, dur, 24, ws=(wp, need))[0] == 0
    refused("workspace", codes, ln, dur, 24, ws=(wp, need - 1))
    refused("workspace", codes, ln, dur, 24, ws=(wp + 128, need))
    refused("overflow", codes, ln, dur, 2 ** 31 // UP, ws=(wp, need), wav_elems=64)
    assert c_forward(eng, codes, ln, dur, 24)[0] == 0  # and the engine still serves
    # dn_voc_durations on a model built without a duration predictor
    nodur = {k: v for k, v in CFG.items() if k != "dur_predictor_params"}
    plain = V.CodeHiFiGANEngine(edge_sd, nodur, dtype="f32")
    out = torch.full((B, T), -77, dtype=torch.int32, device=eng.device)
    sums = torch.full((B,), -77, dtype=torch.int32, device=eng.device)
    wp, wn = plain._ws_for(B, T)
    with torch.cuda.device(eng.device):
        rc = lib.dn_voc_durations(plain.handle, codes.data_ptr(), ln.data_ptr(), B, T, out.data_ptr(), sums.data_ptr(), wp, wn, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == DN_EINVAL and b"no duration predictor" in lib.dn_last_error()
    assert (out == -77).all() and (sums == -77).all()
    rc, wav, wl = c_forward(plain, codes, ln, None, T)
    assert rc == 0 and wl.tolist() == [12 * UP, 5 * UP]
