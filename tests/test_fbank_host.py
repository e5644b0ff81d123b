"""CPU checks of the Kaldi fbank + CMVN front end (include/diffnorm_hip.h, the fbank section; csrc/fbank.hip's host code): the
definition (tests/fbank_ref.py's float64 restatement) against an independent implementation, the host tables against that
restatement, frame counts, the struct layout, the refusals and the compiled kernels' resources.  No GPU is needed."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import fbank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffnorm_hip.h")


@pytest.fixture(scope="module")
def lib():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_restatement_against_an_independent_implementation():
    """The float64 restatement against transformers.audio_utils configured the way SeamlessM4TFeatureExtractor configures it for
    Kaldi compliance (torchaudio and pyKaldi are not installed beside this project): log-mel within 1e-5 (1.1e-7 measured), mel
    weights within 1e-12 (equal when measured)."""
    pytest.importorskip("transformers")
    from transformers.audio_utils import mel_filter_bank, spectrogram, window_function

    x = np.round(3000.0 * np.random.default_rng(0).standard_normal(32000))
    mel = mel_filter_bank(num_frequency_bins=257, num_mel_filters=80, min_frequency=20, max_frequency=8000, sampling_rate=16000, norm=None,
                          mel_scale="kaldi", triangularize_in_mel_space=True)
    ours = R.mel_banks(80, 512, 16000.0)
    w_err = np.abs(mel.T - ours).max()
    theirs = spectrogram(x, window_function(400, "povey", periodic=False), frame_length=400, hop_length=160, fft_length=512, power=2.0, center=False,
                         preemphasis=0.97, mel_filters=mel, log_mel="log", mel_floor=R.FLOOR, remove_dc_offset=True, dtype=np.float64).T
    got = R.fbank64(x)
    assert got.shape == theirs.shape == (198, 80)
    err = np.abs(got - theirs).max()
    print(f"float64 restatement vs transformers.audio_utils: log-mel {err:.2e}, mel weights {w_err:.2e}")
    assert err <= 1e-5 and w_err <= 1e-12


def _ulps(a32, ref64):
    """|a32 - ref| in units of the float32 spacing at float32(ref)."""
    r32 = ref64.astype(np.float32)
    return np.abs(a32.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.maximum(np.abs(r32), np.float32(1e-30)))


@pytest.mark.parametrize("sr,n_mels", [(16000.0, 80), (8000.0, 40)])
def test_tables_are_the_float32_rounding_of_the_restatement(lib, sr, n_mels):
    from diffnorm_amd import fbank

    cfg = fbank.FbankConfig(sample_rate=sr, n_mels=n_mels)
    W, S, N = R.sizes(sr)
    assert (cfg.frame_length, cfg.frame_shift, cfg.fft_size) == (W, S, N)
    window, mel, tw = fbank.host_tables(cfg)
    assert _ulps(window, R.povey_window(W)).max() <= 1
    ref = R.mel_banks(n_mels, N, sr)
    assert mel.shape == ref.shape and _ulps(mel, ref).max() <= 1
    assert ((mel != 0) == (ref.astype(np.float32) != 0)).all()
    assert ((mel != 0).sum(axis=0) <= 2).all() and (mel[:, -1] == 0).all()
    k = np.arange(N // 2, dtype=np.float64)
    assert _ulps(tw[:, 0], np.cos(2 * np.pi * k / N)).max() <= 1 and _ulps(tw[:, 1], -np.sin(2 * np.pi * k / N)).max() <= 1


def test_frame_counts():
    from diffnorm_amd import fbank

    cfg = fbank.FbankConfig()
    ns = [0, 399, 400, 559, 560, 719, 720]
    assert [fbank.out_frames(cfg, n) for n in ns] == [0, 0, 1, 1, 2, 2, 3]
    assert [R.n_frames(n, 400, 160) for n in ns] == [0, 0, 1, 1, 2, 2, 3]


def test_out_frames_of_the_library(lib):
    """dn_fbank_out_frames through a handle: creating one reads no table and launches nothing, so it needs no GPU."""
    from diffnorm_amd import _lib, fbank

    c = fbank.FbankConfig().c_struct()
    dummy = (C.c_float * 4)()
    tabs = (C.c_void_p * 3)(*[C.addressof(dummy)] * 3)
    h = C.c_void_p()
    _lib.check(lib.dn_fbank_create(C.byref(c), tabs, 3, C.byref(h)), "dn_fbank_create")
    try:
        assert [lib.dn_fbank_out_frames(h, n) for n in (0, 399, 400, 559, 560, 719, 720)] == [0, 0, 1, 1, 2, 2, 3]
        assert lib.dn_fbank_workspace_bytes(h, 3, 16000) > 0
    finally:
        lib.dn_fbank_destroy(h)


def test_struct_layout_matches_header(tmp_path):
    from diffnorm_amd import _lib

    fields = [f for f, _ in _lib.FbankConfig._fields_]
    assert fields == ["sample_rate", "n_mels", "frame_length", "frame_shift", "n_fft", "low_freq", "high_freq", "preemphasis", "remove_dc_offset",
                      "input_scale", "norm_means", "norm_vars", "cmvn"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("size %zu\\n", sizeof(DnFbankConfig));']
    lines += [f'printf("{f} %zu\\n", offsetof(DnFbankConfig, {f}));' for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(_lib.FbankConfig) == int(out["size"])
    for f in fields:
        assert getattr(_lib.FbankConfig, f).offset == int(out[f]), f


@pytest.mark.parametrize("bad,word", [(dict(n_fft=2048), "n_fft"), (dict(n_mels=129), "mel bins"), (dict(high_freq=8000.5), "Nyquist")])
def test_unsupported_configurations_are_refused_on_the_host(lib, bad, word):
    from diffnorm_amd import fbank

    with pytest.raises(ValueError, match=word):
        fbank.FbankConfig(**bad)
    c = fbank.FbankConfig().c_struct()
    for k, v in bad.items():
        setattr(c, k, v)
    window, mel = np.zeros(2048, dtype=np.float32), np.zeros(129 * 1025, dtype=np.float32)
    assert lib.dn_fbank_tables(C.byref(c), window.ctypes.data, mel.ctypes.data) == -1
    assert word.encode() in lib.dn_last_error()


@pytest.mark.parametrize("bad", [dict(dither=1.0), dict(use_energy=True), dict(htk_compat=True), dict(vtln_warp=1.1), dict(window_type="hamming"),
                                 dict(snip_edges=False), dict(subtract_mean=True)])
def test_the_rest_of_the_signature_is_refused_by_name(bad):
    from diffnorm_amd import fbank

    with pytest.raises(ValueError, match=next(iter(bad)).split("_")[0]):
        fbank.FbankConfig(**bad)


def test_fbank_kernels_use_no_scratch():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("check_resources", os.path.join(ROOT, "tools", "check_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.check(["fbank.hip"]) == []


@pytest.fixture(scope="module")
def phases_program(tmp_path_factory):
    """tools/fbank_phases_host.hip built with AddressSanitizer and UBSan on the host side: a stand-alone program with its own main."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("fbank_phases") / "fbank_phases_host"
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "diffnorm_amd", "csrc"), os.path.join(ROOT, "tools", "fbank_phases_host.hip"),
                    "-o", str(exe)], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sr,n_mels,frames", [(16000.0, 80, 21), (8000.0, 40, 35), (32000.0, 128, 9)])
def test_kernel_phases_stepped_on_the_cpu(phases_program, tmp_path, sr, n_mels, frames):
    """The frames kernel's own phases (csrc/fbank.hip, all three transform sizes), stepped thread by thread on the CPU under the host
    sanitizers: no read past the utterance's samples, no out-of-bounds access to the LDS image or the tables (a sanitizer report
    fails the run), and the raw log-mel within 4 x the plain float32 torch restatement's own error against float64 -- the device
    test's bar.  No phase reads what another thread writes in the same phase, so stepping the threads in order is what the barriers
    give on the device."""
    W, S, N = R.sizes(sr)
    x = R.parity_wave(W + S * (frames - 1) + S // 3, 3, sr)
    x.astype(np.float32).tofile(tmp_path / "wave.f32")
    r = subprocess.run([str(phases_program), str(sr), str(n_mels), str(W), str(S), str(N), str(tmp_path / "wave.f32"), str(tmp_path / "raw.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = np.fromfile(tmp_path / "raw.f32", dtype=np.float32).reshape(-1, n_mels).astype(np.float64)
    ref = R.fbank64(x, sr, n_mels)
    assert got.shape == ref.shape == (frames, n_mels)
    err, err32 = np.abs(got - ref).max(), np.abs(R.fbank32_torch(x, sr, n_mels).double().numpy() - ref).max()
    print(f"phases on the CPU, n_fft {N}: {err:.3e} vs float32 restatement {err32:.3e} (ratio {err / err32:.2f})")
    assert err <= 4.0 * err32
