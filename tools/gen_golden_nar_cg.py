#!/usr/bin/env python3
"""tests/golden/nar_cg.npz: classifier-free-guided mask-predict decoding by the REAL reference classes (leaf-loaded by
oracle/ref_loader.load_reference_nar) -- TransformerUnitDecoder.forward(inference_mode=True), TransformerUnitDecoder.cg_forward
(research/TranSpeech/nar_transformer.py:123-183) and fairseq's _skeptical_unmasking -- on the small decoder and portable weights of
tests/golden/nar_decoder.npz (oracle/gen_golden_nar.build_reference_model).  The loop around them restates
research/TranSpeech/nat_gen.py:196-236 (gen_with_units: that function also loads audio, k-means and a vocoder, none of which decoding
touches): scores start from zero in every iteration, masked positions take the arg-max of log_softmax(cond + s (cond - null)),
all but the last iteration re-mask the lowest-scoring (n_nonpad - 2) (1 - (step + 1) / n) positions.
Stored: inputs, the first iteration's cond / null logits, tokens / scores / predicted after every iteration for n = 4 at s = 0.5
(scripts/s2ut/eval_cg.sh) and 3.0 (the top of its commented sweep).  One target length is 1 (n_nonpad = 2: boundary 0).
Before writing, every iteration is checked for decisions a different arithmetic could flip (tests/nar_cg_ref.margins).
Run where the reference tree is present: python tools/gen_golden_nar_cg.py"""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import nar_cg_ref as G  # noqa: E402
import ref_loader  # noqa: E402
from gen_golden import save  # noqa: E402
from gen_golden_nar import build_reference_model  # noqa: E402
from gen_golden_nar_configs import CFG, encoder_out  # noqa: E402

N_ITERS, SCALES, ENC_SEED = 4, (0.5, 3.0), 811


def main():
    R = ref_loader.load_reference_nar()
    model, d = build_reference_model(R)
    unmask = sys.modules["fairseq.models.nat.cmlm_transformer"]._skeptical_unmasking
    B, S = 4, 23
    src_lens = torch.tensor([23, 9, 17, 14])
    tgt_lens = torch.tensor([14, 6, 1, 9])
    enc = encoder_out(B, S, src_lens, ENC_SEED)
    out = {"enc_out": enc["encoder_out"][0], "src_lens": src_lens, "tgt_lens": tgt_lens, "n_iters": N_ITERS, "scales": torch.tensor(SCALES),
           "null_token": d.bos()}
    fresh = lambda: {k: [x.clone() for x in v] for k, v in enc.items()}  # cg_forward overwrites the dict it is given (:157-158)
    for si, scale in enumerate(SCALES):
        tokens = G.initial_tokens(tgt_lens, CFG)  # prepare_batch (:109-113)
        out[f"s{si}_tok_in"] = tokens.clone()
        for step in range(N_ITERS):  # nat_gen.py:196-236
            scores = tokens.new_full(tokens.shape, 0.0).float()
            masks = tokens == d.unk()
            with torch.no_grad():
                cond, _ = model.decoder(normalize=False, prev_output_tokens=tokens, encoder_out=fresh(), inference_mode=True)
                null, _ = model.decoder.cg_forward(normalize=False, prev_output_tokens=tokens, encoder_out=fresh())
            scaled = cond + scale * (cond - null)
            m_arg, gap, zeros = G.margins(scaled, tokens, step, N_ITERS, d.unk(), d.pad())
            print(f"scale {scale} step {step}: arg-max margin {m_arg:.3e}, boundary gap {gap:.3e}, zero scores {zeros}")
            assert m_arg >= G.MARGIN and gap >= G.MARGIN and zeros == 0, "choose another ENC_SEED"
            if step == 0 and si == 0:
                out["cond0"], out["null0"] = cond, null
            _scores, _tokens = torch.max(torch.log_softmax(scaled, dim=-1), dim=-1)
            tokens = tokens.clone()
            tokens.masked_scatter_(masks, _tokens[masks])
            scores.masked_scatter_(masks, _scores[masks])
            out[f"s{si}_i{step}_pred"] = tokens.clone()
            if step < N_ITERS - 1:
                sk = unmask(scores, tokens.ne(d.pad()), 1 - (step + 1) / N_ITERS)
                tokens.masked_fill_(sk, d.unk())
                scores.masked_fill_(sk, 0.0)
            out[f"s{si}_i{step}_tok"], out[f"s{si}_i{step}_sc"] = tokens.clone(), scores.clone()
    save("nar_cg", **out)


if __name__ == "__main__":
    main()
