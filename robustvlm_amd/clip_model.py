"""Host-side mirror of the reference's model / loss wrappers around the native engine.

Mirrors (same names, argument meaning and error behaviour):
  ClipVisionModel      train/adversarial_training_clip.py:246-257
  ComputeLossWrapper   train/adversarial_training_clip.py:260-274
  compute_loss, l2, ce train/adversarial_training_clip.py:495-528
  compute_acc          train/adversarial_training_clip.py:488-492
  ClassificationModel  CLIP_eval/clip_robustbench.py:50-69
  ClipTextModel        open_clip CLIP.encode_text as called at train/adversarial_training_clip.py:166-170
  ClipVisionTower      llava/model/multimodal_encoder/clip_encoder.py:55-65, 77-90 (feature_select) and
                       open_flamingo/src/factory.py:41, flamingo.py:217,242 (visual(x)[1])

The arithmetic runs in librvlm.so: ``ClipVisionModel.forward`` is a torch.autograd.Function over
rvlm_vit_forward / rvlm_vit_backward_input (so even the reference's unmodified ``pgd`` can
differentiate through it), the losses go through rvlm_loss_grad.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib as L
from .engine import VitEngine, _require_cuda, _f32c
from .resize import BicubicResize
from .text_engine import TextEngine


class _EncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vision, engine: VitEngine, output_normalize: bool):
        need = ctx.needs_input_grad[0]
        emb = engine.forward(vision, None, output_normalize, save=need)
        ctx.engine = engine
        ctx.generation = engine.generation
        return emb

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("the engine's saved activations were overwritten by a later forward; "
                               "backward must follow its forward (one graph at a time)")
        return eng.backward_input(grad_out), None, None


class ClipVisionModel(torch.nn.Module):
    """forward(vision in [0,1], output_normalize) = visual(Normalize(vision)) [L2-normalised].

    ``model`` is a :class:`VitEngine` (the native replacement of open_clip's ``model.visual``);
    ``normalize`` (a torchvision-Normalize-like object with .mean/.std) is checked against the
    constants baked into the engine, because Normalize is fused into the patch-embed load."""

    def __init__(self, model: VitEngine, args=None, normalize=None):
        super().__init__()
        if not isinstance(model, VitEngine):
            raise TypeError("ClipVisionModel expects a robustvlm_amd.VitEngine as `model`")
        self.model = model
        self.args = args
        self.normalize = normalize
        if normalize is not None and hasattr(normalize, "mean"):
            m = tuple(float(v) for v in normalize.mean)
            s = tuple(float(v) for v in normalize.std)
            if max(abs(a - b) for a, b in zip(m + s, model.mean + model.std)) > 1e-7:
                raise ValueError("normalize constants differ from the ones fused into the engine")

    def forward(self, vision, output_normalize):
        _require_cuda(vision, "vision")
        return _EncodeFn.apply(vision, self.model, bool(output_normalize))


class _TokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vision, engine: VitEngine, depth: int, ln_post: bool):
        need = ctx.needs_input_grad[0]
        tok = engine.forward_tokens(vision, None, depth=depth, ln_post=ln_post, save=need)
        ctx.engine = engine
        ctx.generation = engine.generation
        return tok

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("the engine's saved activations were overwritten by a later forward; "
                               "backward must follow its forward (one graph at a time)")
        return eng.backward_input_tokens(grad_out), None, None, None


class ClipVisionTower(torch.nn.Module):
    """The tower as a VLM reads it: ``forward(vision in [0,1])`` returns token features, differentiable with respect to
    ``vision`` (rvlm_vit_forward_tokens / rvlm_vit_backward_input_tokens behind a ``torch.autograd.Function``).

    ``select_layer``: -2 = the residual stream with the last resblock dropped (LLaVA: ``CLIPVisionTower.feature_select`` on
    ``hidden_states[-2]``, clip_encoder.py:55-65, 77-90), -1 = after every block (OpenFlamingo: ``visual(x)[1]`` with
    ``output_tokens``, factory.py:41, flamingo.py:217,242).  ``select_feature``: 'patch' drops the class row (``[:, 1:]``),
    'cls_patch' keeps it.  ``ln_post`` normalises every token first (open_clip releases that do so for the tokens they
    return).  ``normalize``: as for :class:`ClipVisionModel` - Normalize is fused into the engine, so the images passed here
    are in [0,1], and an object with .mean / .std is checked against the engine's constants.

    One live graph per engine: the backward reads the activations its forward left in the engine, so a second forward
    (of this tower or any other use of the engine) before ``backward`` makes the backward raise."""

    def __init__(self, model: VitEngine, select_layer: int = -2, select_feature: str = "patch", ln_post: bool = False,
                 normalize=None):
        super().__init__()
        if not isinstance(model, VitEngine):
            raise TypeError("ClipVisionTower expects a robustvlm_amd.VitEngine as `model`")
        if select_layer not in (-1, -2):
            raise ValueError(f"select_layer {select_layer!r}: -2 (LLaVA) or -1 (all blocks)")
        if select_feature not in ("patch", "cls_patch"):
            raise ValueError(f"Unexpected select feature: {select_feature}")          # clip_encoder.py:88
        if select_layer == -2 and model.cfg.layers < 2:
            raise ValueError("select_layer = -2 needs a tower of at least two blocks")
        if getattr(model, "mixed", False):
            raise ValueError(f"token passes run on the plain precisions ('bf16', 'fp32', 'x3'), not on {model.precision!r}")
        self.model = model
        self.select_layer = int(select_layer)
        self.select_feature = select_feature
        self.ln_post = bool(ln_post)
        self.normalize = normalize
        if normalize is not None and hasattr(normalize, "mean"):
            m = tuple(float(v) for v in normalize.mean)
            s = tuple(float(v) for v in normalize.std)
            if max(abs(a - b) for a, b in zip(m + s, model.mean + model.std)) > 1e-7:
                raise ValueError("normalize constants differ from the ones fused into the engine")

    @property
    def depth(self) -> int:
        return self.model.cfg.layers + 1 + self.select_layer

    @property
    def hidden_size(self) -> int:
        return self.model.cfg.width

    @property
    def num_patches(self) -> int:
        return self.model.n_tokens - 1

    def feature_select(self, tokens):
        return tokens[:, 1:] if self.select_feature == "patch" else tokens

    def forward(self, vision, output_normalize=False):
        """``output_normalize`` exists for pgd()'s calling convention (forward(x, output_normalize=...)); tokens are never
        L2-normalised, so anything but False is an error."""
        if output_normalize:
            raise ValueError("ClipVisionTower returns token features; output_normalize does not apply")
        _require_cuda(vision, "vision")
        return self.feature_select(_TokensFn.apply(vision, self.model, self.depth, self.ln_post))


class ClipTextModel(torch.nn.Module):
    """``encode_text(text, normalize=False)`` with open_clip's signature over a :class:`TextEngine` - the text half of
    the frozen ``model_orig`` (train/adversarial_training_clip.py:166-170, CLIP_eval/eval_utils.py:74-78).  Forward only:
    the result carries no graph.  ``text`` is what ``open_clip.tokenize`` returns, on the CPU or the device."""

    def __init__(self, model: TextEngine):
        super().__init__()
        if not isinstance(model, TextEngine):
            raise TypeError("ClipTextModel expects a robustvlm_amd.TextEngine as `model`")
        self.model = model

    def encode_text(self, text, normalize: bool = False):
        return self.model.encode(text, normalize=bool(normalize))

    def forward(self, text, normalize: bool = False):
        return self.encode_text(text, normalize)


# --------------------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------------------
class _LossFn(torch.autograd.Function):
    """loss value + d loss/d embedding from one rvlm_loss_grad call."""

    @staticmethod
    def forward(ctx, emb, ref, targets, kind: int, reduction: int, logit_scale: float):
        lib = L.load()
        e = _f32c(emb)
        r = _f32c(ref)
        B, D = e.shape
        Ccls = int(r.shape[1]) if kind == L.LOSS_CE else 0
        per = torch.empty(B, dtype=torch.float32, device=e.device)
        scalar = torch.empty(1, dtype=torch.float32, device=e.device)
        d_emb = torch.empty_like(e)
        scratch = torch.empty(B * Ccls + D * Ccls, dtype=torch.float32, device=e.device) if Ccls else None
        tg = targets.detach().to(torch.int64).contiguous() if kind == L.LOSS_CE else None
        if tg is not None and tg.numel() and (int(tg.min()) < 0 or int(tg.max()) >= Ccls):
            raise IndexError(f"Target out of bounds for {Ccls} classes")           # F.cross_entropy's check
        with torch.cuda.device(e.device):
            L.check(lib.rvlm_loss_grad(kind, reduction, e.data_ptr(), r.data_ptr(), L.ptr(tg), None, B, D, Ccls,
                                       float(logit_scale), per.data_ptr(), scalar.data_ptr(),
                                       d_emb.data_ptr(), None, L.ptr(scratch), L.stream_ptr()),
                    "rvlm_loss_grad")
        ctx.save_for_backward(d_emb)
        ctx.reduction = reduction
        return scalar.reshape(()) if reduction == L.RED_MEAN else per

    @staticmethod
    def backward(ctx, g):
        (d_emb,) = ctx.saved_tensors
        if ctx.reduction == L.RED_MEAN:
            return d_emb * g, None, None, None, None, None
        return d_emb * g.reshape(-1, 1), None, None, None, None, None


class _TokenL2Fn(torch.autograd.Function):
    """per-image sum over rows and width of (tokens - ref)^2 and its gradient from one rvlm_tokens_l2_loss_grad call."""

    @staticmethod
    def forward(ctx, tok, ref):
        lib = L.load()
        t, r = _f32c(tok), _f32c(ref)
        B, n, W = t.shape
        per = torch.empty(B, dtype=torch.float32, device=t.device)
        d = torch.empty_like(t)
        scratch = torch.empty(B * ((n + 7) // 8), dtype=torch.float32, device=t.device)
        with torch.cuda.device(t.device):
            L.check(lib.rvlm_tokens_l2_loss_grad(t.data_ptr(), r.data_ptr(), B, n, W, L.TOKENS_ALL, L.RED_NONE, d.data_ptr(), None, 0,
                                                 per.data_ptr(), None, scratch.data_ptr(), None, L.stream_ptr()),
                    "rvlm_tokens_l2_loss_grad")
        ctx.save_for_backward(d)
        return per

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return d * g.reshape(-1, 1, 1), None


def l2(out, targets, reduction="none"):
    """squared l2, not divided by the latent dimension (…clip.py:509-521).  Token features [B, n, W] (a
    :class:`ClipVisionTower`'s output): summed over rows and width per image, on the device kernel of the token loss."""
    assert out.shape == targets.shape, f"{out.shape} != {targets.shape}"
    assert out.shape[0] > 1
    _require_cuda(out, "out")
    if out.dim() == 3:
        per = _TokenL2Fn.apply(out, targets)
        return per.mean() if reduction == "mean" else per
    red = L.RED_MEAN if reduction == "mean" else L.RED_NONE
    return _LossFn.apply(out, targets, None, L.LOSS_L2, red, 1.0)


class _CeLogitsFn(torch.autograd.Function):
    """F.cross_entropy(logits, targets, reduction) and d loss / d logits from one rvlm_ce_logits call."""

    @staticmethod
    def forward(ctx, logits, targets, reduction: int):
        lib = L.load()
        lg = _f32c(logits)
        B, Ccls = lg.shape
        tg = targets.detach().to(torch.int64).contiguous()
        if tg.numel() and (int(tg.min()) < 0 or int(tg.max()) >= Ccls):
            raise IndexError(f"Target out of bounds for {Ccls} classes")           # F.cross_entropy's check
        per = torch.empty(B, dtype=torch.float32, device=lg.device)
        scalar = torch.empty(1, dtype=torch.float32, device=lg.device)
        d_logits = torch.empty_like(lg)
        with torch.cuda.device(lg.device):
            L.check(lib.rvlm_ce_logits(lg.data_ptr(), tg.data_ptr(), B, Ccls, reduction, per.data_ptr(),
                                       scalar.data_ptr(), d_logits.data_ptr(), None, L.stream_ptr()), "rvlm_ce_logits")
        ctx.save_for_backward(d_logits)
        ctx.reduction = reduction
        return scalar.reshape(()) if reduction == L.RED_MEAN else per

    @staticmethod
    def backward(ctx, g):
        (d_logits,) = ctx.saved_tensors
        if ctx.reduction == L.RED_MEAN:
            return d_logits * g, None, None
        return d_logits * g.reshape(-1, 1), None, None


def ce(out, targets, reduction="mean"):
    """cross entropy on logits (…clip.py:523-528), on the device kernel of librvlm."""
    assert out.shape[0] == targets.shape[0], (out.shape, targets.shape)
    assert out.shape[0] > 1
    _require_cuda(out, "out")
    if reduction not in ("mean", "none", "sum"):
        raise ValueError(f"reduction {reduction} not supported")
    if reduction == "sum":
        return _CeLogitsFn.apply(out, targets, L.RED_NONE).sum()
    return _CeLogitsFn.apply(out, targets, L.RED_MEAN if reduction == "mean" else L.RED_NONE)


def compute_loss(loss_str, embedding, targets, embedding_orig, logit_scale,
                 embedding_text_labels_norm=None, reduction="mean"):
    """…clip.py:495-507."""
    _require_cuda(embedding, "embedding")
    if loss_str == "l2":
        return l2(out=embedding, targets=embedding_orig, reduction=reduction)
    if loss_str == "ce":
        assert embedding.shape[0] == targets.shape[0], (embedding.shape, targets.shape)
        assert embedding.shape[0] > 1
        if reduction not in ("mean", "none"):
            raise ValueError(f"reduction {reduction} not supported")
        red = L.RED_MEAN if reduction == "mean" else L.RED_NONE
        # logits = embedding @ (logit_scale * T), F.cross_entropy - fused in rvlm_loss_grad
        return _LossFn.apply(embedding, embedding_text_labels_norm, targets, L.LOSS_CE, red,
                             float(logit_scale))
    raise ValueError(f"loss {loss_str} not supported")


class ComputeLossWrapper:
    """…clip.py:260-274."""

    def __init__(self, embedding_orig, embedding_text_labels_norm, reduction="mean", loss=None,
                 logit_scale=100.):
        self.embedding_orig = embedding_orig
        self.embedding_text_labels_norm = embedding_text_labels_norm
        self.reduction = reduction
        self.loss_str = loss
        self.logit_scale = logit_scale

    def __call__(self, embedding, targets):
        return compute_loss(loss_str=self.loss_str, embedding=embedding, targets=targets,
                            embedding_orig=self.embedding_orig, logit_scale=self.logit_scale,
                            embedding_text_labels_norm=self.embedding_text_labels_norm,
                            reduction=self.reduction)

    # what the fused device loops need
    def fused_spec(self):
        if self.loss_str == "l2":
            return "l2", self.embedding_orig
        if self.loss_str == "ce":
            return "ce", self.embedding_text_labels_norm
        raise ValueError(f"loss {self.loss_str} not supported")


@torch.no_grad()
def compute_acc(logits, targets):
    """…clip.py:488-492."""
    preds_clean = logits.max(dim=1)[1].detach()
    return (preds_clean.eq(targets).sum() / targets.shape[0]).item() * 100


class _HeadLogitsFn(torch.autograd.Function):
    """logits = (emb @ T) * scale on rvlm_head_logits / rvlm_head_logits_bwd (clip_robustbench.py:66-68)."""

    @staticmethod
    def forward(ctx, emb, T, scale: float):
        lib = L.load()
        e, t = _f32c(emb), _f32c(T)
        B, D = e.shape
        assert t.dim() == 2 and t.shape[0] == D, f"text embedding must be [{D}, C], got {tuple(t.shape)}"
        logits = torch.empty(B, t.shape[1], dtype=torch.float32, device=e.device)
        with torch.cuda.device(e.device):
            L.check(lib.rvlm_head_logits(e.data_ptr(), t.data_ptr(), B, D, t.shape[1], float(scale), logits.data_ptr(),
                                         L.stream_ptr()), "rvlm_head_logits")
        ctx.save_for_backward(t)
        ctx.scale = float(scale)
        return logits

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        lib = L.load()
        g = _f32c(g)
        B, Ccls = g.shape
        d_emb = torch.empty(B, t.shape[0], dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            L.check(lib.rvlm_head_logits_bwd(g.data_ptr(), t.data_ptr(), B, t.shape[0], Ccls, ctx.scale,
                                             d_emb.data_ptr(), L.stream_ptr()), "rvlm_head_logits_bwd")
        return d_emb, None, None


class ClassificationModel(torch.nn.Module):
    """Zero-shot head on the native encoder (CLIP_eval/clip_robustbench.py:50-69):
    logits = normalize(encode_image(Normalize(resizer(x)))) @ T  [* exp(logit_scale) = 100].

    ``resizer``: None, a :class:`BicubicResize` (the reference's ``Resize(224, BICUBIC, antialias=False)``: where its result is
    the engine's own resolution it runs INSIDE the engine - fused into the patch embedding, and the device attack loops work
    at the input's resolution), or any other callable (applied as given; the attacks then take their generic route)."""

    def __init__(self, model, text_embedding, args=None, input_normalize=None, resizer=None,
                 logit_scale=True, logit_scale_value: float = 100.0):
        super().__init__()
        self.vision = model if isinstance(model, ClipVisionModel) else ClipVisionModel(model, args,
                                                                                        input_normalize)
        self.model = self.vision.model
        self.args = args
        self._identity_resizer = resizer is None
        self.resizer = resizer if resizer is not None else (lambda x: x)
        self.text_embedding = text_embedding
        self.logit_scale = logit_scale
        self.logit_scale_value = float(logit_scale_value)

    def engine_input_size(self, vision):
        """(h, w) if the engine itself can run this model's resizer on ``vision`` (``VitEngine.set_input_size``): a
        :class:`BicubicResize` that takes ``vision``'s size, not above the model's, to exactly (image_size, image_size).
        None otherwise - the identity resizer included."""
        if not isinstance(self.resizer, BicubicResize) or not isinstance(vision, torch.Tensor) or vision.dim() != 4:
            return None
        h, w = int(vision.shape[-2]), int(vision.shape[-1])
        img = self.model.cfg.image_size
        if vision.shape[1] != 3 or vision.dtype != torch.float32 or max(h, w) > img or self.model.trainable:
            return None
        if self.resizer.output_size(h, w) != (img, img):
            return None
        return h, w

    @contextlib.contextmanager
    def engine_route(self, vision):
        """For the device attack loops: yields True if they can take ``vision`` as it is - the resizer is the identity, or the
        engine runs it (the handle's input size is then set for the duration of the block and restored after, exceptions
        included) - and False for any other resizer."""
        fused = self.engine_input_size(vision)
        if fused is None:
            yield self._identity_resizer
        else:
            with self.model.input_size_of(*fused):
                yield True

    def forward(self, vision, output_normalize=True):
        assert output_normalize
        mb = self.model.max_batch
        if vision.shape[0] > mb and not (torch.is_grad_enabled() and vision.requires_grad):
            # evaluation batches larger than the engine's workspace (AutoAttack's bs=250 on a max_batch=128 engine)
            # are encoded in chunks; a differentiable call must fit (one saved forward per engine).  Chunks are cut
            # BEFORE the resizer so that each image passes through it exactly once
            return torch.cat([self.forward(vision[i:i + mb]) for i in range(0, vision.shape[0], mb)], 0)
        fused = self.engine_input_size(vision)
        if fused is not None and not (torch.is_grad_enabled() and vision.requires_grad):
            # prediction passes (Square, FAB, AutoAttack's clean pass): the engine's fused front end, nothing kept
            with self.model.input_size_of(*fused):
                embedding_norm_ = self.vision(vision, True)
        else:
            vision = self.resizer(vision)
            embedding_norm_ = self.vision(vision, True)
        return _HeadLogitsFn.apply(embedding_norm_, self.text_embedding,
                                   self.logit_scale_value if self.logit_scale else 1.0)
