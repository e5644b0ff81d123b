"""diffnorm_amd: MI355X-native (gfx950) implementation of DiffNorm's latent-diffusion denoising hot path.

Layout: csrc/ (HIP kernels + C-ABI engine -> libdiffnorm_hip.so), _lib.py (ctypes binding), ops.py
(op-level wrappers), packing.py (state-dict -> packed weights), engine.py (engine handles),
scheduler.py (noise schedules), metrics.py (edit distance, unit / word / character error rates, BLEU), latent_module.py (host mirror of the reference modules),
fairseq_plugin/ (register_model / register_task / register_criterion surface).
"""
__version__ = "0.1.0"

_ENGINES = {"Resampler": "resample", "FbankEngine": "fbank", "HubertFeatureReader": "hubert", "AsrTranscriber": "asr",
            "KMeansQuantizer": "hubert", "KMeansTrainer": "kmeans", "learn_kmeans": "kmeans",
            "ErrorRate": "metrics", "edit_distance": "metrics", "reduce_units": "metrics", "unit_error_rate": "metrics", "wer": "metrics",
            "cer": "metrics", "BleuScore": "metrics", "bleu_stats": "metrics", "bleu": "metrics", "unit_bleu": "metrics"}


def __getattr__(name):
    """The engines by name, imported at first use (importing the package stays as light as it was)."""
    if name in _ENGINES:
        import importlib

        return getattr(importlib.import_module("." + _ENGINES[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
