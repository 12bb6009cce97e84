"""Drop-in for the reference's `models` package (models/__init__.py): `from models import StofNet, ..., GradPeak`
(main.py:18) resolves unchanged.  StofNet, GradPeak and the Zonzini baselines (ZonziniNetSmall / ZonziniNetLarge:
inference, and with the opt-in `train_route = 'kernels'` training, stofnet_amd/zonzini_training.py; the class default None
still raises where a graph would be recorded, 'aten' runs the module's own layers) run on the gfx950 kernels (stofnet_amd); EDSR_1D(1, 64, B, r | 64) and ESPCN_1D(r <= 64) run inference
on the gfx950 kernels of csrc/riders.hip and keep the stock ATen route with the SampleShuffle1D kernel for training and
for other widths (stofnet_amd/baselines.py); SincNet runs on the gfx950 kernels for the option dict of
main.py (inference only; SincNet() without options raises NotImplementedError); WaveUnet(n_layers = 1 .. 12,
channels_interval=16), the configuration of main.py, runs inference on the gfx950 kernels of csrc/waveunet.hip and trains
on the stock ATen route (stofnet_amd/waveunet.py; another channels_interval, the reference's default WaveUnet() included,
raises NotImplementedError); Kuleshov(input_length >= 641, output_length), the last comparison network of the paper's
table, runs inference on the gfx950 kernels of csrc/kuleshov.hip and trains on the stock ATen route
(stofnet_amd/kuleshov.py; num_layers other than 4, for which the reference's forward fails too, and Kuleshov() without
lengths raise NotImplementedError)."""
from stofnet_amd import EDSR_1D, ESPCN_1D, GradPeak, Kuleshov, SincNet, StofNet, WaveUnet, ZonziniNetLarge, ZonziniNetSmall  # noqa: F401
from stofnet_amd.stofnet import SemiGlobalBlock  # noqa: F401
