"""The LOW side of the split-fp16 range, for the record (profiles/range_contract.jsonl): the pair rescaling of
tests/range_contract_inputs.py with k = 0, -2, ..., -16 pushes one interior activation (the hidden activation behind conv2's
leaky ReLU; the pooled SemiGlobalBlock tensor) into fp16's subnormal range while its consumer's weights grow by 2^|k| -- the
split's absolute loss (<= 2^-25 per operand) meets a consumer that amplifies it, and no range guard can see that.  Per k: the
stage's amplitude (float64 oracle), the error of 'f16x3' and of the fp32 mode against the float64 oracle (max |difference| /
max |y|) and whether the arg-max indices agree.  fp32 is invariant to the bit (tests/test_gpu_range_contract.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import range_contract_inputs as rc
from stofnet_amd import StofNet

dev = torch.device('cuda:0')
rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())
x = rc.exact_input(8, 400)
base = rc.base_state_dict('fused', 4)
truth = rc.forward(base, x, 4, 'fused').numpy()
out_dir = os.environ.get('OUT_DIR') or os.path.join(ROOT, 'out')      # run records, as the tools/*.sh scripts keep them
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, 'range_contract.jsonl'), 'w') as f:
    for spec in ('hid2', 'sgb'):
        for k in range(0, -18, -2):
            sd = rc.rescale(base, spec, k)
            amp = float(np.abs(rc.stages(sd, x, 4, 'fused')[rc.target_stage(spec)]).max())
            e = {'rescaling': spec, 'stage': rc.target_stage(spec), 'k': k, 'stage_max_abs': amp, 'input': '[8,1,400] bursts, r=4',
                 'unit': 'max |y - float64 oracle| / max |y|'}
            for prec in ('f16x3', 'fp32'):
                m = StofNet(upsample_factor=4, precision=prec)
                m.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()}, strict=True)
                y = m.to(dev).eval()(torch.from_numpy(x).to(dev)).cpu().numpy()
                e[prec + '_err'] = rel(y, truth)
                e[prec + '_argmax_equal'] = bool(np.array_equal(y[:, 0].argmax(-1), truth[:, 0].argmax(-1)))
            e['f16x3_within_map_tol_1e-5'] = e['f16x3_err'] < 1e-5
            f.write(json.dumps(e) + '\n')
            print(json.dumps(e), flush=True)
