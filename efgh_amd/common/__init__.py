from .fuse import Fused, fuse  # noqa: F401  (the function: its module is sys.modules['efgh_amd.common.fuse'])
from .score import Score, candidates_around, score, stage_poses  # noqa: F401  (likewise: sys.modules['efgh_amd.common.score'])
from .score_soft import Refined, refine, score_soft  # noqa: F401  (likewise: sys.modules['efgh_amd.common.score_soft'])
