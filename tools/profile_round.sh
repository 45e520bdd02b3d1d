# Round profile (run on the GPU box through gpurun): kernel stats of the whole bench, PMC traffic of the two roofline
# kernels (separate --pmc passes, --kernel-trace only), the per-layer timeline of the temporal stack, the kernel make-up of
# the two deployed ticks (B = 1: classifier-free and classifier guidance), the default bench.
R=${R:-r06}
export OUT=${OUT:-profile_out}     # the records of this run (the ones kept are copied to profiles/); profile_train.sh writes there too
mkdir -p $OUT
export HIP_FORCE_DEV_KERNARG=1     # as the package sets it at import (under the profiler the GPU is initialised before Python starts)
rm -rf $OUT/${R}_stats $OUT/${R}_stats2 $OUT/${R}_pmc_fetch $OUT/${R}_pmc_write $OUT/${R}_tconv_trace
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
# kernel stats of the bench: ONE stream for the perception pass (ADX_RESNET_STREAMS=1 ADX_PERCEPTION_AHEAD=0), so that a kernel's
# duration in the summary is its own (bench.py's roofline.avg_launch_ms_rocprof); then the same command as the product runs it
# (two sub-batch streams + the pass stream: concurrent kernels share the chip and their durations overlap)
ADX_RESNET_STREAMS=1 ADX_PERCEPTION_AHEAD=0 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_stats -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-deployed > $OUT/${R}_bench_under_rocprof.json 2> $OUT/${R}_bench_under_rocprof.err
rm -rf $OUT/${R}_stats2
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_stats2 -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-deployed --no-train > $OUT/${R}_bench_under_rocprof_two_streams.json 2> $OUT/${R}_bench_under_rocprof_two_streams.err
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/${R}_pmc_fetch -- python3 tools/pmc_kernels.py > $OUT/${R}_pmc_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/${R}_pmc_write -- python3 tools/pmc_kernels.py > $OUT/${R}_pmc_write.log 2>&1
rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_tconv_trace -- python3 tools/bench_tconv.py > $OUT/${R}_tconv_layers_hostclock.log 2>&1
python tools/trace_chunks.py $OUT/${R}_tconv_trace > $OUT/${R}_tconv_layers.txt
rm -rf $OUT/${R}_tick_free $OUT/${R}_tick_cls
rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_tick_free -- python3 tools/tick_timeline.py run > $OUT/${R}_tick_run.log 2>&1
MODE=classifier rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_tick_cls -- python3 tools/tick_timeline.py run >> $OUT/${R}_tick_run.log 2>&1
python tools/tick_timeline.py analyze $OUT/${R}_tick_free > $OUT/${R}_tick_free_b1.txt
python tools/tick_timeline.py analyze $OUT/${R}_tick_cls > $OUT/${R}_tick_classifier_b1.txt
# the training step: kernel table, the activation-layout levels A/B, idle time of the traced step, host clock
rm -rf $OUT/prof_tr $OUT/${R}_tr_trace
bash tools/profile_train.sh > $OUT/${R}_train_step_kernels.txt 2>&1
cp $(ls -t $OUT/prof_tr/*/*kernel_stats.csv | head -1) $OUT/${R}_train_kernel_stats.csv
[ -n "$AB_TRAIN_CELLS" ] && python tools/ab_env_train.py ADX_TRAIN_CELLS 0 1 2 3 4 5 > $OUT/${R}_ab_train_cells.txt 2>&1
NOSYNC=1 rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_tr_trace -- python3 tools/train_time.py > /dev/null 2>&1
python tools/train_gaps.py $OUT/${R}_tr_trace > $OUT/${R}_train_gaps.txt 2>&1
rm -rf $OUT/${R}_tr_trace
python3 tools/host_times.py 2>/dev/null | tail -22 > $OUT/${R}_train_host_times.txt
python bench.py --full > $OUT/${R}_bench_default.json 2> $OUT/${R}_bench_default.err
ls $OUT/${R}_*/*/ | head -30
tail -c 400 $OUT/${R}_bench_default.json
