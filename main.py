#!/usr/bin/env python3
"""Inference entry point with the reference's `python main.py key=value ...` interface
(reference main.py:29-34,133-177,292-347), running the MI355X-native hot path.

What it keeps: config.yaml + CLI merge, seeding (main.py:39-41), the model switch
(stofnet / edsr / espcn / zonzini / kuleshov / sincnet / unet / gradpeak, main.py:133-167), checkpoint lookup by file-name prefix with strict
load_state_dict (main.py:173-177), the eval loop's `model(frame)` -> `mask2coords` ->
`toa_rmse` sequence (main.py:314,320,347), and with `evaluate=False` the training loop
(main.py:199-289: Gaussian-mask loss, AdamW, CosineAnnealingLR per epoch, EarlyStopping on the
summed validation loss, checkpoint `<run_name>_rf-scale<rf>_epoch_<e>.pth`, main.py:423-426) on the
HIP training kernels, for model=stofnet, model=edsr and model=espcn (EDSR_1D, ESPCN_1D: torch loss and optimizer on the module's
autograd boundary, exact fp32; `train_route=kernels` runs the backward pass on the gfx950 kernels, `train_route=aten` on stock ATen
layers; model=zonzini trains the same way with `zonzini_loss`, the reference's main.py:233-241, its route switch being
`train_route=kernels|aten` too; model=sincnet and model=unet
train with the same lines and switch, train-mode BatchNorm included; model=kuleshov does so only with `kuleshov_train=True`
(its Dropout masks are then a pure function of (seed, step), see stofnet_amd/kuleshov_training.py) and evaluates only without
it; every other model evaluates only); launched under torch.distributed.run it becomes DDP (batch sharded over ranks,
one flat gradient all-reduce per step over RCCL).  `augment=True` puts the reference's training transforms in front of every
training step (main.py:49,54,82: CropChannelData(crop_ratio) + AddNoise(snr_db) on chirp data, AddNoise alone otherwise) as
one launch of the device kernel (stofnet_amd/augment.py); `shuffle=True` reorders the training rows every epoch
(main.py:110).  What it drops: datasets (absent from the reference
mount) and wandb.  Inputs come from `input_file` (.npy) or from synthetic echoes with known onsets.
"""
import json
import os
import random
import sys
import time
from pathlib import Path

import numpy as np
import torch

script_path = Path(__file__).parent.resolve()
sys.path.insert(0, str(script_path))

from stofnet_amd import EDSR_1D, ESPCN_1D, GradPeak, Kuleshov, SincNet, StofNet, WaveUnet, ZonziniNetLarge, ZonziniNetSmall, mask2coords  # noqa: E402
from stofnet_amd import config as config_mod                     # noqa: E402
from stofnet_amd.metrics import toa_rmse                         # noqa: E402


class RunLog:
    """The reference's `logging` switch (main.py:113-130): falsy = no logging at all; otherwise the run is logged under that
    group name -- to wandb when it is installed (same project, metric names and summary keys as main.py:115-130,349-373,
    415-421), else to `<run_name>_<group>.jsonl` next to the script with the same keys, so downstream table scripts find
    the same fields."""

    SUMMARY_KEYS = ('model_name', 'total_parameters', 'total_jaccard', 'total_inference_time', 'total_distance_mean',
                    'total_distance_std')

    def __init__(self, cfg):
        self.enabled = bool(cfg.logging) and int(os.environ.get('RANK', '0')) == 0
        self.wb = None
        self.path = None
        self.name = str(cfg.run_name)
        if not self.enabled:
            return
        try:
            import wandb
            self.wb = wandb.init(project='StofNet', resume='allow', anonymous='must', config=cfg.to_container(),
                                 group=str(cfg.logging))
            self.name = self.wb.name
        except ImportError:
            self.path = script_path / f'{cfg.run_name}_{cfg.logging}.jsonl'
            self.path.write_text('')

    def log(self, record):
        if not self.enabled:
            return
        if self.wb is not None:
            self.wb.log(record)
        else:
            with open(self.path, 'a') as f:
                f.write(json.dumps({k: (float(v) if hasattr(v, '__float__') else v) for k, v in record.items()}) + '\n')

    def summary(self, values):
        if not self.enabled:
            return
        if self.wb is not None:
            for k, v in values.items():
                self.wb.summary[k] = v
            self.wb.finish()
        else:
            self.log({'summary': values})


def load_frames(cfg):
    if cfg.input_file:
        arr = np.load(cfg.input_file).astype(np.float32)
        if arr.ndim == 4:                                                # PALA loader output [B, waves, C, S]: main.py:301 takes wave wv_idx = 1 (main.py:71)
            arr = arr[:, int(getattr(cfg, 'wave_index', 1))]
        if arr.ndim == 3 and arr.shape[1] > 1:
            # PALA-shaped frames [B, C, S]: NormalizeVol acts on the whole frame (utils/transforms.py:13), then
            # `frame.reshape(-1, S).unsqueeze(1)` (main.py:301) -> [B*C, 1, S]; batch_size keeps counting frames
            arr = arr / np.abs(arr).max(axis=(1, 2), keepdims=True)
            cfg.rows_per_frame = int(arr.shape[1])
            return arr.reshape(-1, 1, arr.shape[-1]), None
        arr = arr[:, None, :] if arr.ndim == 2 else arr
        return arr / np.abs(arr).max(axis=-1, keepdims=True), None     # NormalizeVol (utils/transforms.py:13)
    from stofnet_amd.synth import synth_echo          # deterministic demo inputs only
    x, onsets = synth_echo(int(cfg.num_waveforms), int(cfg.num_samples), seed=int(cfg.seed), return_onsets=True)
    return x, onsets.astype(np.float32)[:, None]


def main(argv=None):
    cfg = config_mod.merge(config_mod.load(str(script_path / 'config.yaml')), config_mod.from_cli(argv))
    torch.manual_seed(cfg.seed)
    random.seed(cfg.seed)
    np.random.seed(cfg.seed)

    frames, gt = load_frames(cfg)
    name = str(cfg.model).lower()
    if name == 'stofnet':
        model = StofNet(upsample_factor=cfg.upsample_factor, precision=cfg.precision)
    elif name == 'edsr':                                                  # main.py:139-142: baselines riding on SampleShuffle1D
        model = EDSR_1D(num_channels=1, num_features=64, num_blocks=8, upscale_factor=cfg.upsample_factor)   # trains: train()
    elif name == 'espcn':
        model = ESPCN_1D(upscale_factor=cfg.upsample_factor)                  # trains: train()
    elif name == 'zonzini':                                               # main.py:135-136: Small on chirp data, else Large
        model = ZonziniNetSmall() if 'chirp' in str(cfg.data_dir).lower() else ZonziniNetLarge()       # trains: train()
    elif name == 'kuleshov':                                              # main.py:137-138
        model = Kuleshov(input_length=int(frames.shape[-1]), output_length=int(frames.shape[-1]) * int(cfg.upsample_factor))
        if not bool(getattr(cfg, 'kuleshov_train', False)):
            cfg.evaluate = True                                           # evaluate only, unless kuleshov_train=True asks for train()
    elif name == 'sincnet':                                               # main.py:143-158
        if cfg.fs is None:
            raise ValueError('model=sincnet needs the sample rate: set the config key fs (Hz of the dataset; the sinc '
                             'layer is built for fs * rf_scale_factor and the checkpoints do not store it)')
        cfg.upsample_factor = 1
        opts = {'input_dim': int(frames.shape[-1]), 'fs': float(cfg.fs) * int(cfg.rf_scale_factor),
                'cnn_N_filt': [128, 128, 128, 1], 'cnn_len_filt': [1023, 11, 9, 7], 'cnn_max_pool_len': [1, 1, 1, 1],
                'cnn_use_laynorm_inp': False, 'cnn_use_batchnorm_inp': False,
                'cnn_use_laynorm': [False, False, False, False], 'cnn_use_batchnorm': [True, True, True, True],
                'cnn_act': ['leaky_relu', 'leaky_relu', 'leaky_relu', 'linear'], 'cnn_drop': [0.0, 0.0, 0.0, 0.0],
                'use_sinc': True}
        model = SincNet(opts)                                             # trains: train()
    elif name == 'unet':                                                  # main.py:44-46,159-160
        cfg.rf_scale_factor = cfg.rf_scale_factor * cfg.upsample_factor
        cfg.upsample_factor = 1
        n_layers = 2 if 'chirp' in str(cfg.data_dir).lower() else 10
        if int(frames.shape[-1]) % (1 << n_layers):
            raise ValueError(f'model=unet with n_layers={n_layers} needs a frame length that is a multiple of '
                             f'{1 << n_layers} (got {int(frames.shape[-1])} samples)')
        model = WaveUnet(n_layers=n_layers, channels_interval=16)             # trains: train()
    elif name == 'gradpeak':
        chirp = 'chirp' in str(cfg.data_dir).lower()
        model = GradPeak(threshold=cfg.th, rescale_factor=cfg.rf_scale_factor,
                         echo_max=1 if chirp else float('inf'), onset_opt=chirp)
        cfg.evaluate = True
    else:
        raise Exception('Model not recognized')
    if 'LOCAL_RANK' in os.environ and str(cfg.device) == 'cuda':          # one process per GPU under torch.distributed.run
        cfg.device = f"cuda:{os.environ['LOCAL_RANK']}"
        torch.cuda.set_device(cfg.device)
    model = model.to(cfg.device)
    model.eval()

    if name != 'gradpeak' and cfg.model_file:
        ckpt_dir = Path(cfg.ckpt_dir) if os.path.isabs(str(cfg.ckpt_dir)) else script_path / cfg.ckpt_dir
        prefix = str(cfg.model_file).split('_')[0]
        paths = [fn for fn in sorted(ckpt_dir.iterdir()) if fn.name.startswith(prefix)] if ckpt_dir.is_dir() else []
        if paths:
            model.load_state_dict(torch.load(str(paths[0]), map_location=cfg.device, weights_only=True))

    log = RunLog(cfg)
    if log.enabled and str(cfg.run_name) == 'local-run':
        cfg.run_name = log.name                                          # the reference names checkpoints after the wandb run
    history = train(model, frames, gt, cfg, log) if (not cfg.evaluate and name in ('stofnet', 'edsr', 'espcn', 'zonzini', 'kuleshov', 'sincnet', 'unet')) else None
    es_all, summary = evaluate(model, name, frames, gt, cfg, log)
    log.summary({'model_name': name, 'total_parameters': int(sum(p.numel() for p in model.parameters())),
                 'total_jaccard': summary.get('total_jaccard'), 'total_inference_time': summary['inference_time'],
                 'total_distance_mean': summary.get('total_distance_mean'), 'total_distance_std': summary.get('total_distance_std')})
    if history is not None:
        summary['train_history'] = history
        if name in ('edsr', 'espcn', 'zonzini', 'kuleshov', 'sincnet', 'unet'):
            summary['train_route'], summary['train_precision'] = model.train_route, 'fp32'
    if int(os.environ.get('RANK', '0')) == 0:
        print(json.dumps(summary))
    return es_all, summary


def zonzini_loss(pred, gt_sample, r):
    """The Zonzini branch of the reference's loss (main.py:233-241, validation :332-342): pred [N, 1] against the ground-truth
    value of each row's first onset, gt_sample [N, K] (slots <= 0 or NaN are empty, main.py:217).

    The onset picked is the slot with the smallest non-zero sample index `round(gt r) // r` (main.py:218,236-239; the first
    such slot on a tie, slot 0 when the row has none, whose value is then 0).  The reference hands `MSELoss` pred [N, 1] and
    the gathered targets t [N, 1, 1]; they broadcast to [N, N, 1] (torch warns), so its loss is the mean over ALL PAIRS,
    sum over n, m of (pred_n - t_m)^2 / N^2, not the row-wise mean.  That value and its gradient are kept."""
    gt = torch.nan_to_num(gt_sample.to(pred.device), nan=0.0)
    gt = torch.where(gt <= 0, torch.zeros_like(gt), gt)                                          # main.py:217
    idx = torch.round(gt * r).long() // int(r)                                                   # main.py:218,236
    idx = torch.where(idx == 0, torch.full_like(idx, 10 ** 12), idx)                             # main.py:238
    t = torch.gather(gt, -1, torch.argmin(idx, dim=-1, keepdim=True)).to(pred.dtype)             # main.py:239-240, [N, 1]
    return ((pred.reshape(1, -1) - t.reshape(-1, 1)) ** 2).mean()                                # main.py:241


def epoch_batches(n_rows, bs, epoch, rank, world, shuffle=False, seed=0):
    """[(global batch index, rows of that batch)] of `rank` for one epoch.  Without `shuffle` the rows are slices in file
    order.  With it they index a fresh permutation of the training rows (the DataLoader's shuffle of main.py:110), drawn
    from (seed, epoch) alone and before rank_batches: every rank sees the same order and takes its own batches of it."""
    from stofnet_amd.sharding import rank_batches
    mine = rank_batches(n_rows // bs, rank, world)                       # the same number of steps on every rank
    if not shuffle:
        return [(b, slice(b * bs, (b + 1) * bs)) for b in mine]
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(n_rows)
    return [(b, order[b * bs:(b + 1) * bs]) for b in mine]


def train(model, frames, gt, cfg, log=None):
    """main.py:199-289 + 403-410 + 423-426 on the HIP training kernels (stofnet_amd/training.py).

    StofNet trains through `StofNetTrainer` or, with trainer=autograd, through the reference's own torch lines on the module's
    autograd boundary.  EDSR_1D (model=edsr) and ESPCN_1D (model=espcn) always take those torch lines, in exact fp32 whatever
    `train_precision` says: with train_route=kernels `loss.backward()` runs the gfx950 kernels (stofnet_amd/edsr_training.py,
    stofnet_amd/espcn_training.py), with train_route=aten the same loop runs on stock ATen layers.  The Zonzini nets
    (model=zonzini) take the same lines and the same switch (stofnet_amd/zonzini_training.py) with `zonzini_loss` as their loss.
    SincNet (model=sincnet, upsample_factor 1) takes them too (stofnet_amd/sincnet_training.py): its BatchNorm layers run in train
    mode, so every step also updates their running statistics, and under DDP each rank normalises with its own batch statistics
    (the reference has no SyncBatchNorm either).  WaveUnet (model=unet, upsample_factor 1) does the same through
    stofnet_amd/waveunet_training.py, and Kuleshov (model=kuleshov with kuleshov_train=True) through
    stofnet_amd/kuleshov_training.py, where the Dropout masks of the kernel route are drawn from (cfg.seed, step, rank).

    With `augment=True` every training batch goes through stofnet_amd.augment.Augment first (generator: seed = cfg.seed,
    rank = RANK, one `call` per step) and the ground truth moves with the crop window before it becomes sample indices.
    The held-out validation tail is NOT augmented.  This differs from the reference on purpose: there the validation split
    shares the noisy dataset, but early stopping with delta = 1e-6 needs a loss that does not move with the noise draw."""
    import torch.distributed as dist
    from stofnet_amd.sharding import agree_any
    from stofnet_amd.training import StofNetTrainer
    if gt is None:
        raise RuntimeError('training needs ground-truth onsets (synthetic echoes or a labelled input)')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group('nccl', device_id=torch.device(cfg.device))
    zonzini = isinstance(model, (ZonziniNetSmall, ZonziniNetLarge))
    routed = zonzini or isinstance(model, (EDSR_1D, ESPCN_1D, Kuleshov, SincNet, WaveUnet))          # the baselines with a `train_route` switch
    tr = None if routed else StofNetTrainer(model, lr=cfg.lr, weight_decay=cfg.weight_decay, lambda_value=cfg.lambda_value,
                                            mask_amplitude=cfg.mask_amplitude, kernel_size=cfg.kernel_size, sigma=cfg.sigma,
                                            precision=cfg.train_precision)
    r, bs = int(cfg.upsample_factor), int(cfg.batch_size)
    n_val = max(bs, int(frames.shape[0] * 0.1) // bs * bs)              # held-out tail for early stopping
    tr_x, tr_gt = frames[:-n_val], gt[:-n_val]
    va_x, va_gt = frames[-n_val:], gt[-n_val:]
    shuffle = bool(getattr(cfg, 'shuffle', False))
    aug = None
    if bool(getattr(cfg, 'augment', False)):
        from stofnet_amd.augment import Augment
        chirp = 'chirp' in str(cfg.data_dir).lower()                     # main.py:49,54 crop + noise | main.py:82 noise
        aug = Augment(snr_db=float(cfg.snr_db), crop_ratio=float(cfg.crop_ratio) if chirp else None, seed=int(cfg.seed),
                      rank=rank)
    best, bad, history = float('inf'), 0, []
    restore_deterministic = None

    def gt_true_of(g):
        if zonzini:                                                      # `zonzini_loss` takes the ground truth as it is
            return torch.from_numpy(g).to(cfg.device) if isinstance(g, np.ndarray) else g
        if isinstance(g, np.ndarray):
            g = torch.from_numpy(np.nan_to_num(g, nan=0.0)).to(cfg.device)
        else:
            g = torch.nan_to_num(g, nan=0.0)
        g = torch.where(g <= 0, torch.zeros_like(g), g)                  # main.py:217
        return torch.round(g.unsqueeze(1) * r).long()                    # main.py:218

    autograd = routed or str(getattr(cfg, 'trainer', 'fused')) == 'autograd'
    if autograd:
        # the reference's own training lines (main.py:179-180,184-188,221-248,288) on the module's autograd boundary:
        # torch loss, torch.optim.AdamW, CosineAnnealingLR; `loss.backward()` runs the stof_train_* kernels
        import torch.nn.functional as F
        from stofnet_amd.mask2samples import coords2mask
        from stofnet_amd.training import allreduce_max_, allreduce_mean_, gaussian_kernel
        if routed:
            route = str(getattr(cfg, 'train_route', 'kernels'))
            if route not in ('kernels', 'aten'):
                raise ValueError(f"train_route must be 'kernels' or 'aten' (got {route!r})")
            model.train_route = route
            if isinstance(model, Kuleshov) and route == 'aten':
                # MIOpen: algorithms whose results repeat, so that two runs compare; put back when training ends (below)
                restore_deterministic = torch.backends.cudnn.deterministic
                torch.backends.cudnn.deterministic = True
        else:
            model.train_precision = str(cfg.train_precision)
        optimizer = torch.optim.AdamW(model.parameters(), lr=float(cfg.lr), weight_decay=float(cfg.weight_decay))
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, int(cfg.epochs))
        loss_mse, loss_l1 = torch.nn.MSELoss(reduction='mean'), torch.nn.L1Loss(reduction='mean')
        gauss = torch.tensor(gaussian_kernel(int(cfg.kernel_size), cfg.sigma), dtype=torch.float32,
                             device=cfg.device).unsqueeze(0).unsqueeze(0)

        def torch_loss(masks_pred, gt_true, sharded=True):
            if zonzini:
                return zonzini_loss(masks_pred, gt_true, r)                                      # main.py:233-241
            masks_true = coords2mask(gt_true, masks_pred)                                        # main.py:228
            blur = F.conv1d(masks_true, gauss, padding=int(cfg.kernel_size) // 2)                # main.py:229
            bmax = blur.max().reshape(1)
            blur = blur / (allreduce_max_(bmax) if sharded else bmax)                            # main.py:230 (whole batch, all ranks)
            blur = blur * float(cfg.mask_amplitude)                                              # main.py:231
            return (loss_mse(masks_pred.squeeze(1), blur.squeeze(1).float()) +
                    loss_l1(masks_pred.squeeze(1), torch.zeros_like(masks_pred.squeeze(1))) * float(cfg.lambda_value))   # main.py:232

        def autograd_step(frame, gt_true):
            masks_pred = model(frame)                                                            # main.py:221
            loss = torch_loss(masks_pred, gt_true)
            optimizer.zero_grad()                                                                # main.py:246
            loss.backward()                                                                      # main.py:247
            if world > 1:                                                                        # DDP: mean of the shard gradients
                for prm in model.parameters():
                    allreduce_mean_(prm.grad)
            optimizer.step()                                                                     # main.py:248
            return loss.detach(), masks_pred.detach()

    # validation loss (main.py:322-326): the loss kernels of the trainer, or the same torch lines where there is none
    val_loss = tr.loss if tr is not None else (lambda pred, g: torch_loss(pred, g, sharded=False))
    for e in range(int(cfg.epochs)):
        if not autograd:
            tr.set_lr_cosine(e, int(cfg.epochs), float(cfg.lr))          # CosineAnnealingLR stepped per epoch
        model.train()
        tot = 0.0
        mine = epoch_batches(tr_x.shape[0], bs, e, rank, world, shuffle, int(cfg.seed))
        for b, sl in mine:
            step = autograd_step if autograd else tr.train_step
            frame, g = torch.from_numpy(tr_x[sl]).to(cfg.device), tr_gt[sl]
            if aug is not None:
                frame, g, _ = aug(frame, torch.from_numpy(g).to(cfg.device))
            loss, _ = step(frame, gt_true_of(g))
            tot += float(loss)
            if log is not None and log.enabled:
                log.log({'train_step': e * len(mine) + (b - rank) // world + 1, 'train_loss': float(loss)})      # main.py:251-255
        if not autograd:
            tr.raise_if_overflow()           # split-fp16 training: the range guard's sticky word, once per epoch (fp32: never set)
        model.eval()
        val = 0.0
        with torch.no_grad():
            for b0 in range(0, va_x.shape[0] - bs + 1, bs):
                pred = model(torch.from_numpy(va_x[b0:b0 + bs]).to(cfg.device))
                val += float(val_loss(pred, gt_true_of(va_gt[b0:b0 + bs])))
        lr_now = optimizer.param_groups[0]['lr'] if autograd else tr.lr
        if autograd:
            scheduler.step()                                                                                # main.py:288
        history.append({'epoch': e, 'lr': lr_now, 'train_loss': tot / max(len(mine), 1), 'val_loss': val})
        if rank == 0:
            print(json.dumps(history[-1]))
        if log is not None:
            log.log({'lr': lr_now, 'epoch': e})                                                              # main.py:282-286
        if val < best - float(cfg.delta):                                # EarlyStopping (utils/early_stop.py)
            best, bad = val, 0
        else:
            bad += 1
        if agree_any(bad >= int(cfg.patience), device=cfg.device):       # every rank leaves at the same epoch
            break
    if restore_deterministic is not None:
        torch.backends.cudnn.deterministic = restore_deterministic       # the evaluation that follows chooses its algorithms as ever
    if rank == 0 and cfg.ckpt_dir:
        ckpt_dir = Path(cfg.ckpt_dir) if os.path.isabs(str(cfg.ckpt_dir)) else script_path / cfg.ckpt_dir
        ckpt_dir.mkdir(exist_ok=True)
        path = ckpt_dir / f"{cfg.run_name}_rf-scale{cfg.rf_scale_factor}_epoch_{e + 1}.pth"
        torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)
        print(json.dumps({'saved': str(path)}))
    return history


def evaluate(model, name, frames, gt, cfg, log=None):
    bs = int(cfg.batch_size) * int(getattr(cfg, 'rows_per_frame', 1))      # PALA: a batch of B frames is B*C rows (main.py:301)
    results, times = [], []
    with torch.no_grad():
        for b0 in range(0, frames.shape[0] - bs + 1, bs):          # drop_last=True (main.py:111)
            frame = torch.from_numpy(frames[b0:b0 + bs]).to(cfg.device)
            torch.cuda.synchronize()
            tic = time.perf_counter()
            out = model(frame)
            if name in ('stofnet', 'edsr', 'espcn', 'kuleshov', 'sincnet', 'unet'):          # main.py:318-320
                es = mask2coords(out, window_size=cfg.nms_win_size, threshold=cfg.th,
                                 upsample_factor=cfg.upsample_factor)
            else:
                es = out
            torch.cuda.synchronize()
            times.append((time.perf_counter() - tic) / bs)
            if name == 'stofnet' and getattr(model, 'precision', '') == 'f16x3':
                model.raise_if_overflow()                    # the fast mode alone has no fp32 re-run ('auto' does)
            results.append(es.reshape(bs, -1).cpu().numpy())
            if log is not None:
                log.log({'val_step': b0 // bs + 1, 'inference_time': times[-1]})                            # main.py:349-356
    kmax = max(r.shape[1] for r in results)
    es_all = np.concatenate([np.pad(r, ((0, 0), (0, kmax - r.shape[1]))) for r in results], 0)
    summary = {'model': name, 'waveforms': int(es_all.shape[0]), 'inference_time': float(np.mean(times)),
               'waveforms_per_s': float(1.0 / np.mean(times))}
    if gt is not None:
        # toa_rmse (main.py:347) on the device kernel
        errs = toa_rmse(torch.from_numpy(gt[:es_all.shape[0]]).to(cfg.device), torch.from_numpy(es_all).to(cfg.device),
                        tol=cfg.etol).cpu()
        dist_all = errs[:, 0].numpy()
        with np.errstate(all='ignore'):
            summary['total_distance_mean'] = float(np.nanmean(dist_all)) if np.isfinite(dist_all).any() else float('nan')
            summary['total_distance_std'] = float(np.std(dist_all[~np.isnan(dist_all)])) if np.isfinite(dist_all).any() else float('nan')
            summary['total_jaccard'] = float(np.nanmean(errs[:, 3].numpy()))
        if log is not None:
            for k, row in enumerate(errs.numpy()):                                                          # main.py:359-373
                log.log({'val_idx': k, 'val_toa_distance': row[0], 'val_toa_precision': row[1], 'val_toa_recall': row[2],
                         'val_toa_jaccard': row[3], 'val_toa_true_positive': row[4], 'val_toa_false_positive': row[5],
                         'val_toa_false_negative': row[6]})
    return es_all, summary


if __name__ == '__main__':
    main()
