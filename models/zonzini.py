"""models/zonzini.py of the reference on the gfx950 kernels (inference only)."""
from stofnet_amd.zonzini import ZonziniNetLarge, ZonziniNetSmall  # noqa: F401
