set -o pipefail
O=${OUT_DIR:-out}/affn; mkdir -p $O
timeout -k 10 600 python -u -m pytest tests/test_gpu_gru.py tests/test_backward_golden.py -m gpu -x -v -p no:cacheprovider --timeout 300 --timeout-method thread > $O/pytest.log 2>&1; rc=$?; tail -4 $O/pytest.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err || { tail -5 $O/bench.err; exit 1; }
python -c "import json;d=json.load(open('$O/bench.json'));print(d['value'], {k: v['value'] for k, v in d['configs'].items()}, d.get('gru_section'))"
