set -x
O=${OUT_DIR:-out/r6c}
mkdir -p $O
python -m pytest tests/test_gpu_full_depth.py tests/test_hosted_pipelines.py -m gpu -q -x -s -k "28_steps or hosted or stock" > $O/pytest_depth_hosted.txt 2>&1
tail -25 $O/pytest_depth_hosted.txt
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
python - $O/bench_default.json <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print({k:d[k] for k in ('value','ms_per_step','step_ms_by_kind','end_to_end','speedup_vs_full_token')})
print(d['roofline'].get('frac'), d.get('roofline_attention',{}).get('frac'))
PY
