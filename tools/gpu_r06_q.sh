# Round-6 pass q: InstanceNorm backward in two launches (apply reduces the partials itself):
# bit-identity test, the step parity tests, then the step A/B (IRGAN_IN_BWD_3PASS=1 = old form)
export TMPDIR=/tmp
O=gpurun_out/r06_q; mkdir -p $O
timeout -k 10 600 python -u -m pytest tests/test_gpu_in_bwd_parts.py tests/test_gpu_step.py tests/test_gpu_kernels.py -x -q --timeout 300 --timeout-method thread > $O/pytest.log 2>&1
rc=$?; echo "pytest rc=$rc $(tail -1 $O/pytest.log)"
[ $rc -ne 0 ] && { grep -E "^FAILED|Error|assert" $O/pytest.log | head -20; exit 1; }
for r in 1 2 3; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_on_$r.json 2>/dev/null || { echo "on $r failed"; exit 1; }
  IRGAN_IN_BWD_3PASS=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_off_$r.json 2>/dev/null || { echo "off $r failed"; exit 1; }
done
python - <<PY
import json
for t in ("on", "off"):
    v = [json.load(open("$O/bench_%s_%d.json" % (t, r)))["value"] for r in (1, 2, 3)]
    print(t, v, "mean", round(sum(v) / 3, 1))
PY
echo ALLDONE
