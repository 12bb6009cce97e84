"""utils/beamform.py of the reference: device batches on the gfx950 kernels, numpy arrays on the library's host entry."""
from stofnet_amd.beamform import bf_das, bf_das_rx  # noqa: F401
