"""CLI flags the reference's two models accept.  Upstream inherits them from an unused DiT-style decoder
(reference diff_transformer.py:190-314, called at speech_vae_decoder.py:70 / diff_discrete.py:90); none of
them reaches the hot path, they are accepted so existing command lines keep working."""

_INHERITED = [
    ("--conv-kernel-sizes", dict(type=str, metavar="N")),
    ("--conv-channels", dict(type=int, metavar="N")),
    ("--activation-fn", dict(type=str, default="relu")),
    ("--dropout", dict(type=float, metavar="D")),
    ("--attention-dropout", dict(type=float, metavar="D")),
    ("--activation-dropout", dict(type=float, metavar="D")),
    ("--relu-dropout", dict(type=float, metavar="D")),
    ("--encoder-embed-dim", dict(type=int, metavar="N")),
    ("--encoder-ffn-embed-dim", dict(type=int, metavar="N")),
    ("--encoder-layers", dict(type=int, metavar="N")),
    ("--encoder-attention-heads", dict(type=int, metavar="N")),
    ("--encoder-normalize-before", dict(action="store_true")),
    ("--decoder-embed-dim", dict(type=int, metavar="N")),
    ("--decoder-ffn-embed-dim", dict(type=int, metavar="N")),
    ("--decoder-layers", dict(type=int, metavar="N")),
    ("--decoder-attention-heads", dict(type=int, metavar="N")),
    ("--decoder-normalize-before", dict(action="store_true")),
    ("--share-decoder-input-output-embed", dict(action="store_true")),
    ("--layernorm-embedding", dict(action="store_true")),
    ("--no-scale-embedding", dict(action="store_true")),
    ("--load-pretrained-encoder-from", dict(type=str, metavar="STR")),
    ("--encoder-freezing-updates", dict(type=int, metavar="N")),
    ("--speaker-embed-dim", dict(type=int, metavar="N")),
]


def add_inherited_args(parser):
    for flag, kw in _INHERITED:
        parser.add_argument(flag, **kw)
    # the three flags both model files add after the inherited ones
    parser.add_argument("--input-feat-per-channel", default=80)
    parser.add_argument("--depthwise-conv-kernel-size", default=31)
    parser.add_argument("--input-channels", default=1)
    parser.add_argument("--attn-type", default=None)
    parser.add_argument("--pos-enc-type", default="abs")
    parser.add_argument("--classifier_guidance", type=float, default=1.0)


def add_ema_args(parser):
    """The reference's EMA flags (fairseq/dataclass/configs.py EMAConfig: --store-ema, --ema-decay, --ema-start-update,
    --ema-update-freq, --ema-fp32) plus --hip-sample-from.  The EMA here is always fp32: --ema-fp32 is accepted and ignored;
    --ema-seed-model is not supported.  Added by both archs and both tasks; a parser that already has them is left alone."""
    have = {o for a in parser._actions for o in a.option_strings}
    for flag, kw in (
        ("--store-ema", dict(action="store_true", help="keep an exponential moving average of the trained parameters on the device (one flat fp32 buffer, updated inside the Adam kernel's pass); it is written to checkpoints as extra_state['ema']")),
        ("--ema-decay", dict(type=float, default=0.9999, help="decay of the moving average")),
        ("--ema-start-update", dict(type=int, default=0, help="the EMA copies the model (decay 0) until this many updates")),
        ("--ema-update-freq", dict(type=int, default=1, help="update the EMA every this many model updates")),
        ("--ema-fp32", dict(action="store_true", help="accepted for the reference's command lines: the EMA here is always fp32")),
        ("--hip-sample-from", dict(default="model", choices=["model", "ema"], help="which weights the sampling / inference engine of a model in training holds: the trained parameters, or their EMA (needs --store-ema)")),
    ):
        if flag not in have:
            parser.add_argument(flag, **kw)


def ema_schedule(args):
    """The optim.EmaSchedule of a namespace with --store-ema, else None."""
    if not getattr(args, "store_ema", False):
        return None
    from ...optim import EmaSchedule

    return EmaSchedule(decay=getattr(args, "ema_decay", 0.9999), start_update=getattr(args, "ema_start_update", 0),
                       update_freq=getattr(args, "ema_update_freq", 1))


_ARCH_DEFAULTS = dict(
    attn_type=None, pos_enc_type="abs", classifier_guidance=1.0, encoder_freezing_updates=0, conv_kernel_sizes="5,5",
    conv_channels=1024, conv_version="s2t_transformer", encoder_embed_dim=512, encoder_ffn_embed_dim=2048, encoder_layers=12,
    encoder_attention_heads=8, encoder_normalize_before=True, no_scale_embedding=False, dropout=0.1, activation_fn="relu",
    speaker_embed_dim=256, decoder_layers=6, decoder_attention_heads=8, decoder_normalize_before=True,
    decoder_learned_pos=False, adaptive_softmax_cutoff=None, adaptive_softmax_dropout=0,
    share_decoder_input_output_embed=False, no_token_positional_embeddings=False, adaptive_input=False,
    decoder_layerdrop=0.0, quant_noise_pq=0, length_loss_factor=0.1,
)


def apply_arch_defaults(args):
    """Fills the attributes the reference's base_architecture functions set (speech_vae_decoder.py:101-136)."""
    for k, v in _ARCH_DEFAULTS.items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    for k, src in (("attention_dropout", "dropout"), ("activation_dropout", "dropout"), ("decoder_embed_dim", "encoder_embed_dim"),
                   ("decoder_ffn_embed_dim", "encoder_ffn_embed_dim")):
        if getattr(args, k, None) is None:
            setattr(args, k, getattr(args, src))
    for k, src in (("decoder_output_dim", "decoder_embed_dim"), ("decoder_input_dim", "decoder_embed_dim")):
        if getattr(args, k, None) is None:
            setattr(args, k, getattr(args, src))


def is_training_run(args) -> bool:
    """Is this namespace a training run's (fairseq_cli/train.py: it carries --optimizer / --lr; generation and
    diff_norm_synthesis namespaces do not)?  `--hip-train-engine` / `hip_train_engine=True` forces it.  A training run's model
    switches to the HIP training engine -- ONE flat parameter -- the moment it is moved to the GPU, i.e. before the reference
    trainer snapshots `model.parameters()` into its optimizer (fairseq/trainer.py:292)."""
    if getattr(args, "hip_train_engine", None) is not None:
        return bool(args.hip_train_engine)
    return getattr(args, "optimizer", None) is not None

