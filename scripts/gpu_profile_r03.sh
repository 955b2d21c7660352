# Round-3 profile: every number quoted in DESIGN.md / README.md comes from this script's outputs under profiles/r03_*.
#   gpurun --timeout 2400 -- 'bash scripts/gpu_profile_r03.sh'   then   python scripts/summarize_profile.py r03
# Bench lines, rocprofv3 kernel traces (--kernel-trace --stats) and PMC passes are SEPARATE runs (counters are never
# combined with trace domains; FETCH_SIZE and WRITE_SIZE in passes of their own, MI355X_MICROARCH.md).
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=gpurun_out/prof_r03
rm -rf $O; mkdir -p $O
Q="--no-cpu-baseline --no-other-configs"
python bench.py --full --steps 20 --warmup 5 2>/dev/null > $O/bench_default_driver_form.json
python bench.py --full 2>/dev/null > $O/bench_ifst.json
FARNN_NOFUSE=1 python bench.py --full $Q 2>/dev/null > $O/bench_ifst_two_kernels.json
FARNN_NOREGS=1 FARNN_NOFUSE=1 python bench.py --full $Q 2>/dev/null > $O/bench_ifst_ring_kernel_r02.json
python bench.py --full --full-length $Q 2>/dev/null > $O/bench_ifst_full.json
python bench.py --full --workload ifst_crf $Q 2>/dev/null > $O/bench_ifst_crf.json
FARNN_NOFUSE=1 python bench.py --full --workload ifst_crf $Q 2>/dev/null > $O/bench_ifst_crf_two_kernels.json
python bench.py --full --workload decomp $Q --steps 300 2>/dev/null > $O/bench_decomp.json
FARNN_DECOMP_NOREGS=1 python bench.py --full --workload decomp $Q --steps 300 2>/dev/null > $O/bench_decomp_rows_kernel.json
python bench.py --full --workload decomp --rank 100 --farnn 1 $Q --steps 100 2>/dev/null > $O/bench_decomp_r100_farnn1.json
python bench.py --full --workload decomp --rank 250 --farnn 2 $Q --steps 100 2>/dev/null > $O/bench_decomp_r250_farnn2.json
python bench.py --full --workload decomp1 $Q --steps 100 2>/dev/null > $O/bench_decomp1.json
python bench.py --full --workload decomp0 $Q --steps 100 2>/dev/null > $O/bench_decomp0.json
python bench.py --full --workload fst4 $Q --steps 20 --warmup 3 2>/dev/null > $O/bench_fst4.json
python bench.py --full --workload synth512 --batch 1024 --seqlen 128 --steps 3 --warmup 1 $Q --event-stride 1 2>/dev/null > $O/bench_synth512.json
python bench.py --full --workload train --no-cpu-baseline --steps 50 2>/dev/null > $O/bench_train.json
python bench.py --full --workload train --crf --no-cpu-baseline --steps 50 2>/dev/null > $O/bench_train_crf.json
python bench.py --full --workload train --farnn 2 --crf --rank 250 --no-cpu-baseline --steps 30 2>/dev/null > $O/bench_train_farnn2_crf_r250.json
python scripts/host_inclusive_rate.py 2>/dev/null | grep host-inclusive > $O/host_inclusive.txt
R="--no-cpu-baseline --no-other-configs --no-pipelined --no-parity --event-stride 0"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 bench.py --full --steps 200 --warmup 20 $R > $O/trace.log 2>&1
FARNN_NOFUSE=1 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_two -- python3 bench.py --full --steps 200 --warmup 20 $R > $O/trace_two.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_crf -- python3 bench.py --full --workload ifst_crf --steps 100 --warmup 10 $R > $O/trace_crf.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_decomp -- python3 bench.py --full --workload decomp --steps 100 --warmup 10 $R > $O/trace_decomp.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_fst4 -- python3 bench.py --full --workload fst4 --steps 10 --warmup 2 $R > $O/trace_fst4.log 2>&1
P="--steps 20 --warmup 5 $R"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 bench.py --full $P > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 bench.py --full $P > $O/pmc_write.log 2>&1
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/pmc_l2 -- python3 bench.py --full $P > $O/pmc_l2.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_fst4 -- python3 bench.py --full --workload fst4 --steps 3 --warmup 1 $R > $O/pmc_fetch_fst4.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_synth512 -- python3 bench.py --full --workload synth512 --batch 1024 --seqlen 128 --steps 2 --warmup 1 $R > $O/pmc_fetch_synth512.log 2>&1
i=0
for grp in "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_WAIT_ANY" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"; do
  i=$((i+1))
  for wl in ifst decomp ifst_crf; do
    rocprofv3 --pmc $grp --output-format csv -d $O/sq${i}_$wl -- python3 bench.py --full --workload $wl --steps 10 --warmup 3 $R > $O/sq${i}_$wl.log 2>&1
  done
done
# keep only the small summaries (kernel_stats + counter collection), drop per-dispatch traces > 4 MB
find $O -name '*.csv' -size +4M -delete
find $O -name '*kernel_trace.csv' -delete
du -sh $O
