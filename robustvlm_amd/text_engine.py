"""Python handle of the native CLIP text tower (rvlm_text in include/rvlm.h): ``encode_text`` for the zero-shot / TeCoA head.

Forward only - the reference runs the text tower under ``no_grad`` on the frozen ``model_orig``
(train/adversarial_training_clip.py:150-180, CLIP_eval/eval_utils.py:63-85).  Tokenisation stays with the caller: the
interface takes what ``open_clip.tokenize`` returns ([N, 77] integer ids, SOT 49406, EOT 49407 as the largest id of a
prompt, zero padding)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .config import TextConfig, TEXT_CONFIGS, text_state_dict_shapes
from .engine import _f32c

_PRECISIONS = {"fp32": L.PREC_F32, "bf16": L.PREC_BF16, "x3": L.PREC_F32X3}


class TextEngine:
    """Owns a ``rvlm_text`` handle: converted weights + a workspace sized for ``max_batch`` prompts per native call.

    precision: 'x3' (default: fp32 storage, LayerNorm and attention, the linears as split-bf16 products - the reference
    computes the head in fp32 and the CE loss multiplies it by 100), 'fp32' (fp32 matrix-pipe tiles throughout) or 'bf16'.
    """

    def __init__(self, cfg, state_dict: dict, precision: str = "x3", max_batch: int = 1024, device=None):
        if isinstance(cfg, str):
            cfg = TEXT_CONFIGS[cfg]
        if precision not in _PRECISIONS:
            raise ValueError(f"precision {precision!r} not supported (one of {sorted(_PRECISIONS)})")
        if not torch.cuda.is_available():
            raise L.RvlmError("no ROCm device visible: robustvlm_amd needs an MI355X (no CPU fallback)")
        self.lib = L.load()
        self.cfg, self.precision, self.max_batch = cfg, precision, int(max_batch)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self._h = C.c_void_p()
        c = L.TextConfigC(cfg.vocab, cfg.context, cfg.width, cfg.layers, cfg.heads, cfg.out_dim,
                          L.ACT_QUICK_GELU if cfg.act == "quick_gelu" else L.ACT_GELU, _PRECISIONS[precision],
                          self.max_batch)
        keep = {}
        for k, shp in text_state_dict_shapes(cfg).items():
            if k not in state_dict:
                raise KeyError(f"state_dict is missing {k!r}")
            t = _f32c(state_dict[k]).to(self.device)
            if tuple(t.shape) != tuple(shp):
                raise ValueError(f"{k}: shape {tuple(t.shape)} != {tuple(shp)}")
            keep[k] = t
        w = L.TextWeightsC()
        for f in L.TEXT_TOP_FIELDS:
            setattr(w, f, keep[L.TEXT_TOP_KEYS[f]].data_ptr())
        blocks = (L.BlockWeightsC * cfg.layers)()
        for i in range(cfg.layers):
            for f in L.BLOCK_FIELDS:
                setattr(blocks[i], f, keep[f"transformer.resblocks.{i}.{L.BLOCK_KEYS[f]}"].data_ptr())
        w.blocks_host = C.cast(blocks, C.POINTER(L.BlockWeightsC))
        with torch.cuda.device(self.device):
            L.check(self.lib.rvlm_text_create(C.byref(c), C.byref(w), L.stream_ptr(), C.byref(self._h)), "rvlm_text_create")
        del keep      # the handle holds its own copies

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.rvlm_text_workspace_bytes(self._h))

    @staticmethod
    def active_length(tokens: torch.Tensor) -> int:
        """max_n eot[n] + 1 with eot = tokens.argmax(-1): the positions a causal tower has to evaluate."""
        return int(tokens.argmax(dim=-1).max().item()) + 1

    @torch.no_grad()
    def encode(self, tokens: torch.Tensor, normalize: bool = False, active_len: int | None = None) -> torch.Tensor:
        """``model.encode_text(tokens, normalize)`` -> [N, out_dim] fp32 on the engine's device.

        tokens: [N, context] int32 / int64, on the CPU or the device.  active_len: None = computed here from the tokens,
        0 = the full context, k = the first k positions (must cover every prompt's EOT).  Larger batches are evaluated in
        chunks of ``max_batch`` prompts; the device flag word is read once per call."""
        if not self._h:
            raise L.RvlmError("TextEngine is closed")
        if tokens.dim() != 2 or tokens.shape[1] != self.cfg.context or tokens.shape[0] < 1:
            raise ValueError(f"tokens must be [N >= 1, {self.cfg.context}], got {tuple(tokens.shape)}")
        if tokens.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"tokens must be int32 or int64, got {tokens.dtype}")
        tok = tokens.to(self.device)
        if tokens.dtype == torch.int64 and (int(tok.min()) < 0 or int(tok.max()) >= self.cfg.vocab):
            raise ValueError(f"token id outside [0, {self.cfg.vocab})")      # (before the narrowing to int32 could hide it)
        tok = tok.to(torch.int32).contiguous()
        if active_len is None:
            active_len = self.active_length(tok)
        N = tok.shape[0]
        out = torch.empty(N, self.cfg.out_dim, dtype=torch.float32, device=self.device)
        flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for s in range(0, N, self.max_batch):
                n = min(self.max_batch, N - s)
                L.check(self.lib.rvlm_text_encode(self._h, tok[s:s + n].data_ptr(), n, int(active_len), int(bool(normalize)),
                                                  out[s:s + n].data_ptr(), flags.data_ptr(), L.stream_ptr()), "rvlm_text_encode")
        f = int(flags.item())
        if f & L.FLAG_TOKEN_RANGE:
            raise ValueError(f"token id outside [0, {self.cfg.vocab})")
        if f & L.FLAG_EOT_ACTIVE:
            raise ValueError(f"active_len = {active_len} does not cover the EOT position of every prompt")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rvlm_text_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
