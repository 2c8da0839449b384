"""Evaluation helpers around the zero-shot classifier of BASELINE config 5.

* :func:`compute_accuracy_no_dataloader` - CLIP_eval/eval_utils.py:88-112
* :func:`zeroshot_head`                  - the prompt-ensembling arithmetic of CLIP_eval/clip_robustbench.py:211-224
* :func:`get_text_embeddings`            - CLIP_eval/eval_utils.py:63-85 (one template per class) on the native text tower
* :func:`get_text_embeddings_ensemble`   - CLIP_eval/clip_robustbench.py:211-224 (template ensemble) on the native text tower

Tokenisation stays with the caller: both take the integer ids ``open_clip.tokenize`` returns.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


@torch.inference_mode()
def compute_accuracy_no_dataloader(model, data, targets, device, batch_size=1000):
    """Top-1 accuracy of ``model`` on tensors ``data`` / ``targets`` in chunks of ``batch_size``; the model's
    training flag is restored afterwards."""
    was_training = getattr(model, "training", False)
    if hasattr(model, "eval"):
        model.eval()
    n_total = n_correct = 0
    for s in range(0, data.shape[0], batch_size):
        xb = data[s:s + batch_size].clone().to(device)
        yb = targets[s:s + batch_size].clone().to(device)
        preds = F.softmax(model(xb), dim=1).max(dim=1)[1]
        n_total += yb.size(0)
        n_correct += preds.eq(yb).sum().item()
    if was_training:
        model.train()
    return n_correct / n_total


def zeroshot_head(template_embeddings) -> torch.Tensor:
    """Column-normalised zero-shot head ``T`` [D, C] from text embeddings.

    ``template_embeddings``: tensor [C, n_templates, D] (or a list of C tensors [n_templates_c, D]) of UN-normalised
    text-tower outputs, one row per prompt template.  Per class: normalise every template embedding, average, normalise
    again (clip_robustbench.py:219-222); a single template ([C, 1, D] or [C, D]) gives the 'std' head (:192-209)."""
    cols = []
    if isinstance(template_embeddings, torch.Tensor) and template_embeddings.dim() == 2:
        template_embeddings = template_embeddings.unsqueeze(1)
    for emb in template_embeddings:
        c = F.normalize(emb.float(), dim=-1).mean(dim=0)
        cols.append(c / c.norm())
    T = torch.stack(cols, dim=1)
    assert torch.allclose(F.normalize(T, dim=0), T, atol=1e-6)
    return T


@torch.no_grad()
def get_text_embeddings(text_model, tokens) -> torch.Tensor:
    """``embedding_text_labels_norm`` [D, C] from the token ids [C, context] of one prompt per class:
    ``encode_text(tokens, normalize=True).T`` (CLIP_eval/eval_utils.py:74-80, train/adversarial_training_clip.py:163-172; the
    reference's chunks of 500 prompts are the engine's ``max_batch``).  ``text_model``: a ClipTextModel (or TextEngine)."""
    enc = text_model.encode_text if hasattr(text_model, "encode_text") else text_model.encode
    T = enc(tokens, normalize=True).T.contiguous()
    assert torch.allclose(F.normalize(T, dim=0), T, atol=1e-6)
    return T


@torch.no_grad()
def get_text_embeddings_ensemble(text_model, tokens) -> torch.Tensor:
    """The template-ensemble head [D, C] from token ids [C, n_templates, context] (CLIP_eval/clip_robustbench.py:211-224):
    un-normalised ``encode_text`` of every prompt, then :func:`zeroshot_head`."""
    if tokens.dim() != 3:
        raise ValueError(f"tokens must be [C, n_templates, context], got {tuple(tokens.shape)}")
    enc = text_model.encode_text if hasattr(text_model, "encode_text") else text_model.encode
    C_, n_t, ctx = tokens.shape
    emb = enc(tokens.reshape(C_ * n_t, ctx), normalize=False)
    return zeroshot_head(emb.reshape(C_, n_t, -1))
