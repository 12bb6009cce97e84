"""models/wave_unet.py of the reference on the gfx950 kernels (inference; training on ATen)."""
from stofnet_amd.waveunet import WaveUnet as Model  # noqa: F401
