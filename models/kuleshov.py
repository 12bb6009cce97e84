"""models/kuleshov.py of the reference on the gfx950 kernels (inference; training on ATen)."""
from stofnet_amd.kuleshov import Kuleshov  # noqa: F401
