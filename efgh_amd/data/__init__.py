from .prepare import (ProcessKITTIODOM, ProcessKITTIRAW, ProcessNUSC, ProcessRELLIS, SweepSet,  # noqa: F401
                      accumulation_indices, accumulation_transform, nusc_accumulation_transform, nusc_walk, preproc_gt,
                      preproc_img, preproc_pcd, rand_init_params, voxel_keep)
