from .prepare import (ColorJitter, JitterParams, ProcessKITTIODOM, ProcessKITTIRAW, ProcessNUSC, ProcessRELLIS, SweepSet,  # noqa: F401
                      accumulation_indices, accumulation_transform, color_jitter, nusc_accumulation_transform, nusc_walk, preproc_gt,
                      preproc_img, preproc_pcd, rand_init_params, voxel_keep)
