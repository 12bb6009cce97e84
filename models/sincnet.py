"""models/sincnet.py of the reference on the gfx950 kernels (inference only, the option dict of main.py)."""
from stofnet_amd.sincnet import SincConv, SincNet  # noqa: F401
