#!/bin/bash
# Rehearsal of the N-rank bench path on a ONE-GPU box: both ranks run the real kernels on cuda:0, the collectives
# (barrier, MAX of the step time, index gather, gradient all-reduce) go over gloo because RCCL wants one GPU per rank.
# The figures are NOT throughput claims (two ranks share one GPU); the run shows that every rank-dependent code path
# of bench.py --full executes on the hardware.  Output: $OUT_DIR/rehearse_ranks_one_gpu.jsonl (OUT_DIR default: out)
set -e
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:-out}; mkdir -p $O
out=$O/rehearse_ranks_one_gpu.jsonl
: > $out
python bench.py --gpus 2 --full --steps 5 --warmup 1 --rows 1024 --rehearse-on-one-gpu --no-fp32-extra 2>> $O/rehearse.err >> $out
python bench.py --gpus 2 --full --config C3 --steps 3 --warmup 1 --rows 512 --rehearse-on-one-gpu --no-fp32-extra 2>> $O/rehearse.err >> $out
python bench.py --gpus 2 --full --config C4 --rows 16384 --steps 2 --warmup 1 --rehearse-on-one-gpu 2>> $O/rehearse.err >> $out
python bench.py --gpus 2 --full --config C5 --rows 64 --steps 3 --warmup 1 --rehearse-on-one-gpu 2>> $O/rehearse.err >> $out
python bench.py --gpus 4 --full --steps 3 --warmup 1 --rows 512 --rehearse-on-one-gpu --no-fp32-extra 2>> $O/rehearse.err >> $out
wc -l $out
