"""utils/transforms.py of the reference: device batches on the gfx950 kernel, single samples in numpy."""
from stofnet_amd.transforms import AddNoise, CropChannelData, NormalizeVol  # noqa: F401
