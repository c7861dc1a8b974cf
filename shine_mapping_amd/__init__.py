"""shine_mapping_amd — the SHINE-Mapping SDF training hot path, MI355X (gfx950) native.

Public surface mirrors the reference's modules for this path:
    FeatureOctree   model/feature_octree.py
    Decoder         model/decoder.py
    sdf_bce_loss, get_gradient          utils/loss.py, utils/tools.py
    sdf_diff_loss, batch_ray_rendering_loss   utils/loss.py (main_loss_type sdf_l1 / sdf_l2, dr / dr_neus)
    normal_loss                         the normal_loss_on term (shine_batch.py:192-197) in a form that can be evaluated
    train_step / StepOptions            the fused Tier-B step (one HIP pass) as a torch.autograd.Function
    fused_train_step                    the same launch in raw form (grads written straight into .grad)
    fused_sem_step                      semantic_on: the NLL term of the same batch, one more launch in raw form
    fused_normal_step                   normal_loss_on: the surface-normal term of the same batch, one more launch in raw form
    consistency_loss                    the consistency_loss_on term (shine_batch.py:187-190) with the zero-gradient guard
    fused_consistency_step              consistency_loss_on: the gradient-consistency term on pairs of points, one more launch
    ConsistencyTerm                     ... and its GraphedIteration(consistency=...) form (loop.py)
    fused_time_step                     time_conditioned: the whole step of a 4D map (BCE [+ eikonal] through the 9-wide head), one launch
    fused_ray_step                      ray_loss (dr / dr_neus): the whole step of a ray-rendering map, per-ray render included, one launch
    eval_mesh                           eval/eval_utils.py (mesh metrics against a ground-truth cloud; evaluation.py)
All compute goes through libshine_hip.so (include/shine_hip.h); there is no CPU fallback.
"""
from .decoder import Decoder
from .evaluation import eval_mesh
from .feature_octree import FeatureOctree
from .loop import ConsistencyTerm, RayTerm
from .sampler import RayPool
from .losses import batch_ray_rendering_loss, consistency_loss, get_gradient, normal_loss, sdf_bce_loss, sdf_diff_loss
from .ops import (StepOptions, forward_sdf, fused_consistency_step, fused_normal_step, fused_ray_step, fused_sem_step, fused_time_step,
                  fused_train_step, octree_interp, train_step)

__all__ = ["Decoder", "FeatureOctree", "StepOptions", "forward_sdf", "fused_train_step", "fused_sem_step", "fused_normal_step",
           "train_step", "octree_interp", "sdf_bce_loss", "get_gradient", "sdf_diff_loss", "batch_ray_rendering_loss",
           "normal_loss", "eval_mesh", "consistency_loss", "fused_consistency_step", "ConsistencyTerm",
           "fused_time_step", "fused_ray_step", "RayTerm", "RayPool"]
