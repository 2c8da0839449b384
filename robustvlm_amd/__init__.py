"""robustvlm_amd - MI355X-native adversarial inner loop for RobustVLM-style CLIP fine-tuning.

Host-side mirror of the reference's interface for the hot path; every
arithmetic op runs in the in-tree HIP library ``librvlm.so`` (include/rvlm.h):

    reference                                           here
    train/pgd_train.py::pgd                             robustvlm_amd.pgd
    train/apgd_train.py::apgd_train                     robustvlm_amd.apgd_train
    autoattack/autopgd_base.py::APGDAttack              robustvlm_amd.APGDAttack
    autoattack/fab_pt.py::FABAttack_PT                  robustvlm_amd.FABAttack
    vlm_eval/attacks/utils.py                           robustvlm_amd.attack_utils
    train/adversarial_training_clip.py::ClipVisionModel robustvlm_amd.ClipVisionModel
      ::ComputeLossWrapper/compute_loss/l2/ce           robustvlm_amd.{ComputeLossWrapper,...}
    CLIP_eval/clip_robustbench.py::ClassificationModel  robustvlm_amd.ClassificationModel
    torchvision Resize(224, BICUBIC, antialias=False)   robustvlm_amd.BicubicResize  (the resizer= of the line above)
    open_clip VisionTransformer (third party)           robustvlm_amd.VitEngine
    open_clip CLIP.encode_text (third party)            robustvlm_amd.{TextEngine,ClipTextModel}
    CLIP_eval/eval_utils.py::get_text_embeddings        robustvlm_amd.get_text_embeddings
    vlm_eval/attacks/pgd.py::PGD, apgd.py::APGD, apgd   robustvlm_amd.vlm_attacks.{PGD,APGD,apgd}  (+ TokenLossModel)
    apgd.py::apgd on the token loss, batched            robustvlm_amd.apgd_tokens
"""
from .config import (VitConfig, CONFIGS, CLIP_MEAN, CLIP_STD, random_state_dict, state_dict_shapes, TextConfig, TEXT_CONFIGS,
                     text_state_dict_shapes, random_text_state_dict)
from .engine import VitEngine
from .text_engine import TextEngine
from .clip_model import (ClipVisionModel, ClipVisionTower, ClipTextModel, ComputeLossWrapper, ClassificationModel, compute_loss, l2, ce,
                         compute_acc)
from .attack_utils import project_perturbation, normalize_grad
from .pgd_train import pgd
from .apgd_train import apgd_train
from .autopgd import APGDAttack, APGDAttack_targeted
from .autoattack import AutoAttack, EvaluationState
from .square import SquareAttack
from .fab import FABAttack
from . import vlm_attacks
from .vlm_attacks import TokenLossModel
from .token_attacks import apgd_tokens
from .eval_utils import compute_accuracy_no_dataloader, zeroshot_head, get_text_embeddings, get_text_embeddings_ensemble
from .preprocess import ResizeCenterCropToTensor
from .resize import BicubicResize
from .checkpoint import load_visual_state_dict, load_text_state_dict, CheckpointWriter, resume_paths

__all__ = ["VitConfig", "CONFIGS", "CLIP_MEAN", "CLIP_STD", "random_state_dict", "state_dict_shapes",
           "VitEngine", "ClipVisionModel", "ComputeLossWrapper", "ClassificationModel", "compute_loss",
           "l2", "ce", "compute_acc", "project_perturbation", "normalize_grad", "pgd", "apgd_train",
           "APGDAttack", "APGDAttack_targeted", "AutoAttack", "EvaluationState", "SquareAttack", "FABAttack", "compute_accuracy_no_dataloader", "zeroshot_head", "ResizeCenterCropToTensor", "load_visual_state_dict", "CheckpointWriter", "resume_paths",
           "TextConfig", "TEXT_CONFIGS", "text_state_dict_shapes", "random_text_state_dict", "TextEngine", "ClipTextModel",
           "get_text_embeddings", "get_text_embeddings_ensemble", "load_text_state_dict", "BicubicResize", "ClipVisionTower", "vlm_attacks", "TokenLossModel", "apgd_tokens"]
