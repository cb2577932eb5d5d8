from .efghbackbone import EFGHBackbone  # noqa: F401  (looked up by name, reference main.py:126)
from .builders import BilateralConvFlex  # noqa: F401  (the BCL as a layer: splat -> blur -> slice, nets/bilateralNN.py)
