#!/bin/bash
# smoke(), then the --full bench line (C2 + extras.configs); outputs under $OUT_DIR (default: out)
set -eo pipefail
O=${OUT_DIR:-out}; mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')"
timeout -k 10 500 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err
python - $O/bench_full.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print('C2', d['value'], d['ms_per_step'], d['roofline']['frac'])
for k,c in d['extras']['configs'].items():
    print(k, c.get('value'), c.get('ms_per_step'), c.get('roofline',{}).get('frac'), c.get('roofline',{}).get('algorithmic_frac'), c.get('child_wall_s'), c.get('error'))
PY
