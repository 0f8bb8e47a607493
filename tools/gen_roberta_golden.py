#!/usr/bin/env python3
"""tests/golden/roberta_tiny.npz: a one-layer transformers RobertaModel on the CPU (float32), the fixture of the roberta position
scheme (TextConfig.position_scheme = "roberta").  Needs the installed transformers; the tests read only the .npz.

    python tools/gen_roberta_golden.py [out.npz]

Batch of four 16-token rows: no pad | right-padded | left-padded | a pad id in the middle of the text.  The attention mask is
all ones on the left-padded and interior-pad rows, so their pad tokens carry gradient: the position table's pad row must still
get none (padding_idx), the token-type table has no padding_idx and gets it.

Arrays: "p:<state_dict key>" every parameter; ids, mask; position_ids (transformers' create_position_ids_from_input_ids);
pre (the f32 sum entering the embedding LayerNorm), emb_out (the embedding output), last_hidden_state; R and, for
loss = sum(last_hidden_state[:, 0] * R): d_pre (the gradient at `pre`, from a backward hook) and g_word / g_pos / g_type (the
three table gradients).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, BOS, EOS = 1, 0, 2
B, S = 4, 16


def batch(g):
    tok = lambda n: torch.randint(3, 256, (n,), generator=g)
    ids = torch.full((B, S), PAD, dtype=torch.long)
    ids[0] = torch.cat([torch.tensor([BOS]), tok(S - 2), torch.tensor([EOS])])                        # no pad
    ids[1, :9] = torch.cat([torch.tensor([BOS]), tok(7), torch.tensor([EOS])])                         # right-padded
    ids[2, 5:] = torch.cat([torch.tensor([BOS]), tok(S - 7), torch.tensor([EOS])])                     # left-padded
    ids[3] = torch.cat([torch.tensor([BOS]), tok(4), torch.tensor([PAD]), tok(3), torch.tensor([PAD, PAD]), tok(4),
                        torch.tensor([EOS])])                                                          # pads inside the text
    mask = torch.ones((B, S), dtype=torch.long)
    mask[1] = (ids[1] != PAD).long()
    return ids, mask


def main():
    from transformers import RobertaConfig, RobertaModel
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "roberta_tiny.npz")
    torch.manual_seed(20)
    cfg = RobertaConfig(vocab_size=256, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                        max_position_embeddings=24, type_vocab_size=1, pad_token_id=PAD, layer_norm_eps=1e-5,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, attn_implementation="eager")
    model = RobertaModel(cfg, add_pooling_layer=False).eval()
    with torch.no_grad():       # biases and LayerNorm parameters away from their 0 / 1 initial values
        for n, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape))
    g = torch.Generator().manual_seed(21)
    ids, mask = batch(g)
    R = torch.randn((B, cfg.hidden_size), generator=g)
    emb = model.embeddings
    position_ids = emb.create_position_ids_from_input_ids(ids, PAD)
    seen = {}

    def grab(_, args):
        seen["pre"] = args[0]
        args[0].register_hook(lambda gr: seen.__setitem__("d_pre", gr.detach().clone()))

    h1 = emb.LayerNorm.register_forward_pre_hook(grab)
    h2 = emb.register_forward_hook(lambda _m, _a, o: seen.__setitem__("emb_out", o.detach().clone()))
    last = model(input_ids=ids, attention_mask=mask).last_hidden_state
    h1.remove(), h2.remove()
    (last[:, 0] * R).sum().backward()
    arrays = {"p:" + k: v.detach().numpy() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    arrays.update(ids=ids.numpy(), mask=mask.numpy(), position_ids=position_ids.numpy().astype(np.int32),
                  pre=seen["pre"].detach().numpy(), emb_out=seen["emb_out"].numpy(), last_hidden_state=last.detach().numpy(),
                  R=R.numpy(), d_pre=seen["d_pre"].numpy(), g_word=emb.word_embeddings.weight.grad.numpy(),
                  g_pos=emb.position_embeddings.weight.grad.numpy(), g_type=emb.token_type_embeddings.weight.grad.numpy())
    np.savez_compressed(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(arrays)} arrays; position_ids row 3 = {position_ids[3].tolist()}")


if __name__ == "__main__":
    main()
