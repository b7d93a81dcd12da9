"""groomed_nms_amd -- MI355X-native (gfx950) GrooMeD-NMS layer.

  groomed_nms_amd.groomed_nms   mirror of the reference's lib/groomed_nms.py (differentiable_nms, get_groups, ...)
  groomed_nms_amd.overlaps      mirror of the overlap helpers in lib/core.py / lib/math_3d.py
  groomed_nms_amd.nms           mirror of lib/nms (gpu_nms over the C symbol `_nms`, cpu_nms, py_cpu_nms)
  groomed_nms_amd.nms_others    mirror of lib/nms_others.py
  groomed_nms_amd.detect        the inference post-processing of lib/rpn_util.py::im_detect_3d (detections_from_heads, im_detect_3d)
  groomed_nms_amd.kitti_eval    the KITTI devkit's evaluation (2D / AOS / BEV / 3D AP, all of the reference's variants) in one call
  groomed_nms_amd.kitti_results detections -> the rows the devkit would parse from the result files -> AP, without the files (KittiResults, round6)
  groomed_nms_amd.sampling      the loss's hard-anchor sampling, sample weights and weighted classification term (lib/loss/rpn_3d.py:583-612, 913-1001)
  groomed_nms_amd.regression    the loss's box regression, 2D IoU and uncertainty terms on the sampled foreground (lib/loss/rpn_3d.py:1154-1407)
  groomed_nms_amd.after_nms     the loss's after-NMS block from the heads: selection, decode, GrooMeD-NMS, best box per ground truth, AP / BCE term (lib/loss/rpn_3d.py:721-825, 1091-1148)
  groomed_nms_amd.heads         the fifteen maps of the RPN heads -> cls, prob, bbox_2d, bbox_3d, acceptance rows and the anchor tables (models/densenet121_3d_dilate_decomp_alpha.py:166-245)
  groomed_nms_amd.loss          the reference's RPN_3D_loss as one module: ground-truth records -> targets, sampling, the three terms, total, stats list, one-launch backward (lib/loss/rpn_3d.py)
  groomed_nms_amd.dataset_stats the set-up before the first step: generate_anchors (host) and compute_bbox_stats (GPU) -> conf.anchors, conf.bbox_means, conf.bbox_stds (lib/rpn_util.py:24-216, 547-736)
  groomed_nms_amd.preprocess    the image front end: uint8 BGR images -> mirrored, resized, cropped / padded, normalised float32 RGB planes in one launch; Preprocess, Augmentation (lib/augmentations.py)
  groomed_nms_amd.optim         the optimiser side of the loop: lr_schedule / adjust_lr, FusedSGD (clip, SGD with momentum and weight decay, zero_grad and the `loss > 0` gate in one launch per group, capturable), loss_backprop (lib/core.py:99-170)
  groomed_nms_amd.build         hipcc build of libgroomed_nms_hip.so (C ABI: include/groomed_nms_hip.h)
"""
from .groomed_nms import (differentiable_nms, differentiable_nms_batched, differentiable_nms_from_boxes_batched, differentiable_nms_with_iou2d_batched, differentiable_nms_with_iou3d_batched, soft_sort, pruning_function, sigmoid_numpy,  # noqa: F401
                          cast_to_cpu_cuda_tensor, get_groups, indices_copy, GroomedNMS)
from .detect import detections_from_heads, im_detect_3d  # noqa: F401
from . import kitti_eval  # noqa: F401
from .kitti_eval import evaluate_kitti_results_verbose, run_kitti_eval, evaluate_detections  # noqa: F401
from . import kitti_results  # noqa: F401
from .kitti_results import KittiResults, round6  # noqa: F401
from . import sampling  # noqa: F401
from .sampling import sample_anchors, classification_loss  # noqa: F401
from . import regression  # noqa: F401
from .regression import regression_loss  # noqa: F401
from . import after_nms  # noqa: F401
from .after_nms import after_nms_loss  # noqa: F401
from . import heads  # noqa: F401
from .heads import assemble_heads  # noqa: F401
from . import loss  # noqa: F401
from .loss import RPN_3D_loss, pack_ground_truths, GroundTruths  # noqa: F401
from . import dataset_stats  # noqa: F401
from .dataset_stats import generate_anchors, compute_bbox_stats  # noqa: F401
from . import preprocess  # noqa: F401
from .preprocess import preprocess_images, Preprocess, Augmentation  # noqa: F401
from . import optim  # noqa: F401
from .optim import FusedSGD, lr_schedule  # noqa: F401

__version__ = "0.1.0"
