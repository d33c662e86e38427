# Round-6 pass t: G inc conv with the InstanceNorm statistics fused (conv_c8r STATS) -- tests,
# step parity, step A/B (IRGAN_NO_C8R_STATS=1 = conv + separate statistics pass)
export TMPDIR=/tmp
O=gpurun_out/r06_t; mkdir -p $O
timeout -k 10 600 python -u -m pytest tests/test_gpu_inc_stats.py tests/test_gpu_step.py tests/test_gpu_bf16_parity.py -x -q --timeout 300 --timeout-method thread > $O/pytest.log 2>&1
rc=$?; echo "pytest rc=$rc $(tail -1 $O/pytest.log)"
[ $rc -ne 0 ] && { grep -E "^FAILED|Error|assert" $O/pytest.log | head -20; exit 1; }
for r in 1 2 3; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_on_$r.json 2>/dev/null || { echo "on $r failed"; exit 1; }
  IRGAN_NO_C8R_STATS=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_off_$r.json 2>/dev/null || { echo "off $r failed"; exit 1; }
done
python - <<PY
import json
for t in ("on", "off"):
    v = [json.load(open("$O/bench_%s_%d.json" % (t, r)))["value"] for r in (1, 2, 3)]
    print(t, v, "mean", round(sum(v) / 3, 1))
PY
IRGAN_NO_D_OVERLAP=1 timeout -k 10 300 python tools/layer_times.py > $O/layer_times_serial.txt 2>&1 || { echo lt failed; exit 1; }
grep -E "1x64k7|in_apply:b16@256x256x64" $O/layer_times_serial.txt
echo ALLDONE
