#!/bin/bash
# rocprofv3 evidence of one round, run ON the GPU box from the repo root (gpurun -- 'bash tools/collect_evidence.sh r02'):
# kernel stats of the roofline leg, the three PMC passes over it (FETCH_SIZE, WRITE_SIZE, MfmaUtil: one counter
# set per pass, never together with a trace domain), the kernel trace of the training leg and the kernel stats of
# the default bench command.  Everything lands under gpurun_out/<tag>_*; tools/rocpd_export.py, tools/insitu.py,
# tools/pmc_traffic.py and tools/pmc_summary.py turn it into the files kept under profiles/.
set -o pipefail
tag=${1:-r04}
mkdir -p gpurun_out
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:-$OLDPWD}"
run() { echo "[evidence] $*" >&2; "$@"; }
bench_raw=$(mktemp -d)   # raw rocprofv3 output of the full benchmark (`bench.py --full`): only its conversions are kept
# which sources the profiled library was built from: the converters stamp it into profiles/<tag>_*.json and bench.py
# reports a committed profile as a measurement of the running build only when the hashes agree
python3 -c "from tiny_diffusion_amd import _build; print(_build.source_hash())" > gpurun_out/${tag}_src_sha256.txt
run rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/${tag}_roof -- python3 bench.py --roofline-only > gpurun_out/${tag}_roof.json 2> gpurun_out/${tag}_roof.err && echo roof ok &&
run rocprofv3 --pmc FETCH_SIZE --output-format csv -d gpurun_out/${tag}_pmc_f -- python3 bench.py --roofline-only > /dev/null 2> gpurun_out/${tag}_pmc_f.err && echo pmc_f ok &&
run rocprofv3 --pmc WRITE_SIZE --output-format csv -d gpurun_out/${tag}_pmc_w -- python3 bench.py --roofline-only > /dev/null 2> gpurun_out/${tag}_pmc_w.err && echo pmc_w ok &&
run rocprofv3 --pmc MfmaUtil --output-format csv -d gpurun_out/${tag}_pmc_mfma -- python3 bench.py --roofline-only > /dev/null 2> gpurun_out/${tag}_pmc_mfma.err && echo pmc_mfma ok &&
run rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/${tag}_train -- python3 bench.py --train-only --steps 30 --warmup 5 > gpurun_out/${tag}_train.json 2> gpurun_out/${tag}_train.err && echo train ok &&
run rocprofv3 --kernel-trace --stats --output-format csv -d $bench_raw/trace -- python3 bench.py --full --steps 20 --warmup 5 > $bench_raw/line.json && echo bench ok
rc=$?
# the bf16 mode: kernel stats + one step's timeline of the MNIST leg, every GEMM launch in isolation, L2 counters
rc16=0
if [ $rc -eq 0 ]; then
  run rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/${tag}_bf16 -- python3 tools/gpu_bf16_bench.py mnist 25 > gpurun_out/${tag}_bf16.log 2>&1 && echo bf16 ok
  rc16=$?
fi
# conversions into the files kept under profiles/ (small; done here so that they travel back with gpurun_out/).
# Only after every fp32 leg succeeded: a failed leg must not leave partial files that bench.py would then report
# as a committed profile of this build.
sha=gpurun_out/${tag}_src_sha256.txt
out=gpurun_out/${tag}_profiles
first() { ls $1 2>/dev/null | head -n 1; }          # first match of a glob, or nothing
keep() { [ -n "$1" ] && [ -f "$1" ] && cp "$1" "$2"; }  # copy only what exists
if [ $rc -eq 0 ]; then
  mkdir -p $out
  python3 tools/pmc_traffic.py gpurun_out/${tag}_pmc_f gpurun_out/${tag}_pmc_w $out/${tag}_pmc_hbm_traffic $sha > /dev/null || rc=1
  python3 tools/pmc_summary.py gpurun_out/${tag}_pmc_mfma MfmaUtil $out/${tag}_pmc_MfmaUtil.txt > /dev/null || rc=1
  trace=$(first "gpurun_out/${tag}_train/*/*kernel_trace.csv")
  if [ -n "$trace" ]; then
    python3 tools/insitu.py $trace $out/${tag}_insitu.json $sha > /dev/null || rc=1
    python3 tools/step_timeline.py $trace 10 > $out/${tag}_step_timeline.txt || rc=1
  else
    echo "[evidence] no kernel trace of the training leg" >&2; rc=1
  fi
  keep "$(first "gpurun_out/${tag}_roof/*/*kernel_stats.csv")" $out/${tag}_roofline_leg_kernel_stats.csv || rc=1
  keep "$(first "gpurun_out/${tag}_train/*/*kernel_stats.csv")" $out/${tag}_train_only_kernel_stats.csv || rc=1
  keep "$(first "$bench_raw/trace/*/*kernel_stats.csv")" $out/${tag}_bench_default_kernel_stats.csv || rc=1
  keep gpurun_out/${tag}_roof.json $out/${tag}_roofline_leg.json || rc=1
  keep $bench_raw/line.json $out/${tag}_bench_default_under_rocprof.json || rc=1
  keep $sha $out/ || rc=1
  if [ $rc16 -eq 0 ]; then
    bf=$(first "gpurun_out/${tag}_bf16/*/*kernel_trace.csv")
    if [ -n "$bf" ]; then
      python3 tools/step_timeline.py $bf 10 > $out/${tag}_bf16_step_timeline.txt
      keep "$(first "gpurun_out/${tag}_bf16/*/*kernel_stats.csv")" $out/${tag}_bf16_mnist_kernel_stats.csv
    fi
    python3 tools/gpu_bf16_layers.py mnist > $out/${tag}_bf16_layers_mnist.txt 2>/dev/null || rm -f $out/${tag}_bf16_layers_mnist.txt
    python3 tools/gpu_bf16_layers.py laion64 > $out/${tag}_bf16_layers_laion64.txt 2>/dev/null || rm -f $out/${tag}_bf16_layers_laion64.txt
    bash tools/bf16_layer_counters.sh mnist > /dev/null 2>&1 && keep gpurun_out/bf16_layer_counters_mnist.txt $out/${tag}_bf16_layer_counters_mnist.txt
  fi
fi
# round 4: the reverse step's timeline at n = 16 and n = 64 (after the Winograd / compact-order changes), the
# graph-vs-eager diagnostic behind the capture test, and where the gradient buckets' collectives sit (1-rank RCCL group)
if [ $rc -eq 0 ]; then
  for n in 16 64; do
    run rocprofv3 --kernel-trace --output-format csv -d gpurun_out/${tag}_samp$n -- python3 tools/gpu_sample_trace.py $n 100 > gpurun_out/${tag}_samp$n.log 2>&1
    st=$(first "gpurun_out/${tag}_samp$n/*/*kernel_trace.csv")
    [ -n "$st" ] && python3 tools/sample_timeline.py $st > $out/${tag}_sample_timeline_n$n.txt
    rm -rf gpurun_out/${tag}_samp$n
  done
  python3 tools/gpu_graph_vs_eager.py > $out/${tag}_graph_vs_eager.txt 2>&1 || rm -f $out/${tag}_graph_vs_eager.txt
  # where a workgroup of the Winograd kernels spends its time (in-kernel stamps), and the 13 layers direct vs Winograd
  python3 tools/gpu_wino_phases.py > $out/${tag}_wino_phases.txt 2>/dev/null || rm -f $out/${tag}_wino_phases.txt
  python3 tools/gpu_wino_phases.py --wgrad > $out/${tag}_wino_phases_wgrad.txt 2>/dev/null || rm -f $out/${tag}_wino_phases_wgrad.txt
  python3 tools/gpu_wino_layers.py > $out/${tag}_wino_layers.txt 2>/dev/null || rm -f $out/${tag}_wino_layers.txt
  # matrix / vector pipe counters of the Winograd kernels (one --pmc pass, no trace domain), and the race soak
  bash tools/micro/wino_pipe_counters.sh $tag > /dev/null 2>&1 && keep gpurun_out/${tag}_wino_pipe_counters.txt $out/${tag}_wino_pipe_counters.txt
  python3 tools/gpu_wino_soak.py 50 > $out/${tag}_wino_soak.txt 2>/dev/null || echo "[evidence] Winograd soak FAILED" >&2
  RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 TDX_FORCE_ALLREDUCE=1 \
    rocprofv3 --kernel-trace --output-format csv -d gpurun_out/${tag}_ar -- python3 bench.py --train-only --steps 12 --warmup 3 > gpurun_out/${tag}_ar.log 2>&1
  at=$(first "gpurun_out/${tag}_ar/*/*kernel_trace.csv")
  [ -n "$at" ] && python3 tools/allreduce_timeline.py $at > $out/${tag}_allreduce_timeline.txt 2>&1
  rm -rf gpurun_out/${tag}_ar
fi
# the roofline leg's JSON once more, now that the PMC passes of THIS build exist: its roofline.traffic and
# committed_profile stamp then describe the running build (the first pass above ran before they existed)
if [ $rc -eq 0 ]; then
  cp $out/${tag}_pmc_hbm_traffic.json $out/${tag}_insitu.json $out/${tag}_src_sha256.txt profiles/ 2>/dev/null
  python3 bench.py --roofline-only > $out/${tag}_roofline_leg.json 2> gpurun_out/${tag}_roof2.err || keep gpurun_out/${tag}_roof.json $out/${tag}_roofline_leg.json
fi
# the raw rocprofv3 output directories are large (per-dispatch traces of two 1000-step chains): only the conversions travel back
rm -rf gpurun_out/${tag}_bf16 gpurun_out/${tag}_roof gpurun_out/${tag}_pmc_f gpurun_out/${tag}_pmc_w gpurun_out/${tag}_pmc_mfma gpurun_out/${tag}_train gpurun_out/${tag}_bench
rm -rf $bench_raw
du -sh gpurun_out/${tag}_* 2>/dev/null
[ $rc -eq 0 ] && rc=$rc16
exit $rc
