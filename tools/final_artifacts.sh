#!/bin/bash
# Round-end artefacts on one GPU box: bench lines, kernel statistics of the same command, PMC passes for the traffic file.
#   ARTIFACTS_DIR=<folder> bash tools/final_artifacts.sh   then   python tools/traffic_json.py $ARTIFACTS_DIR/fa_fetch $ARTIFACTS_DIR/fa_write <commit>
#   (ARTIFACTS_DIR defaults to artifacts/ in the repository; tools/collect_artifacts.py reads the same folder)
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${ARTIFACTS_DIR:-artifacts}; mkdir -p "$out"
timeout -k 10 400 python bench.py --full > $out/fa_bench.json 2> $out/fa_bench.err
# (the profiled command is the timed workload alone: with the side legs the statistics would average the colour sweep over the
# 16384^2 and the 32768^2 rasters, whose launches differ in size)
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/fa_trace -- python3 bench.py --no-cpu --no-side > $out/fa_bench_rocprof.json 2> $out/fa_rocprof.err
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $out/fa_fetch -- python3 tools/step_trace.py > $out/fa_f.log 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $out/fa_write -- python3 tools/step_trace.py > $out/fa_w.log 2>&1
timeout -k 10 400 python bench.py --config c4 --no-cpu --no-side > $out/fa_bench_c4.json 2> $out/fa_c4.err
timeout -k 10 200 python bench.py --bands 3 --no-cpu --no-side --steps 3 --warmup 1 > $out/fa_bench_bands3.json 2> $out/fa_b3.err
timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $out/fa_step -- python3 tools/step_trace.py > $out/fa_s.log 2>&1
python3 tools/trace_gaps.py $out/fa_step > $out/fa_step_timeline.txt
OBIA_TRACE_COMPACTNESS=0.25 timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $out/fa_step025 -- python3 tools/step_trace.py > $out/fa_s025.log 2>&1
python3 tools/trace_gaps.py $out/fa_step025 > $out/fa_step_timeline_c025.txt
rm -f $out/fa_trace/*/*kernel_trace.csv $out/fa_step/*/*kernel_trace.csv $out/fa_step025/*/*kernel_trace.csv   # (tens of MB; the statistics are what is kept)
echo artefacts done
