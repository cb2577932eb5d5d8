from .fuse import Fused, fuse  # noqa: F401  (the function: its module is sys.modules['efgh_amd.common.fuse'])
