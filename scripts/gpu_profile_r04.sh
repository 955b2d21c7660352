# Round-4 profile: every number quoted in DESIGN.md / README.md comes from this script's outputs under profiles/r04_*.
#   gpurun --timeout 2700 -- 'bash scripts/gpu_profile_r04.sh'   then   python scripts/summarize_profile.py r04
# Bench lines, rocprofv3 kernel traces (--kernel-trace --stats) and PMC passes are SEPARATE runs (counters are never
# combined with trace domains; FETCH_SIZE and WRITE_SIZE in passes of their own, MI355X_MICROARCH.md).
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=gpurun_out/prof_r04
rm -rf $O; mkdir -p $O
Q="--no-cpu-baseline --no-other-configs"
python bench.py --full --steps 20 --warmup 5 2>/dev/null > $O/bench_default_driver_form.json
python bench.py --full 2>/dev/null > $O/bench_ifst.json
FARNN_NOLABELMAP=1 python bench.py --full $Q 2>/dev/null > $O/bench_ifst_matrix_core_scores.json
FARNN_NOFUSE=1 python bench.py --full $Q 2>/dev/null > $O/bench_ifst_two_kernels.json
python bench.py --full --graph 10 $Q 2>/dev/null > $O/bench_ifst_graph_replay.json
python bench.py --full --full-length $Q 2>/dev/null > $O/bench_ifst_full.json
python bench.py --full --workload ifst --states 104 $Q 2>/dev/null > $O/bench_ifst_s104.json
FARNN_NOFUSE=1 python bench.py --full --workload ifst --states 104 $Q 2>/dev/null > $O/bench_ifst_s104_two_kernels.json
FARNN_NOREGS=1 FARNN_NOFUSE=1 python bench.py --full --workload ifst --states 104 $Q 2>/dev/null > $O/bench_ifst_s104_ring_kernel_r03.json
python bench.py --full --workload ifst --states 128 $Q 2>/dev/null > $O/bench_ifst_s128.json
python bench.py --full --workload ifst_crf $Q 2>/dev/null > $O/bench_ifst_crf.json
FARNN_NOFUSE=1 python bench.py --full --workload ifst_crf $Q 2>/dev/null > $O/bench_ifst_crf_two_kernels.json
python bench.py --full --workload ifst_crf --states 104 $Q 2>/dev/null > $O/bench_ifst_crf_s104.json
FARNN_CV_WIDE=1 python bench.py --full --workload ifst_crf --states 104 $Q 2>/dev/null > $O/bench_ifst_crf_s104_one_launch.json
python bench.py --full --workload decomp $Q --steps 300 2>/dev/null > $O/bench_decomp.json
FARNN_NOLABELMAP=1 python bench.py --full --workload decomp $Q --steps 300 2>/dev/null > $O/bench_decomp_matrix_core_scores.json
python bench.py --full --workload decomp --rank 100 --farnn 1 $Q --steps 100 2>/dev/null > $O/bench_decomp_r100_farnn1.json
python bench.py --full --workload decomp --rank 250 --farnn 2 $Q --steps 100 2>/dev/null > $O/bench_decomp_r250_farnn2.json
FARNN_ROWS_LPR4=1 python bench.py --full --workload decomp --rank 250 --farnn 2 $Q --steps 100 2>/dev/null > $O/bench_decomp_r250_farnn2_four_lanes_r03.json
python bench.py --full --workload decomp --rank 150 --farnn 2 $Q --steps 100 2>/dev/null > $O/bench_decomp_r150_farnn2.json
FARNN_ROWS_LPR4=1 python bench.py --full --workload decomp --rank 150 --farnn 2 $Q --steps 100 2>/dev/null > $O/bench_decomp_r150_farnn2_four_lanes_r03.json
python bench.py --full --workload decomp1 $Q --steps 100 2>/dev/null > $O/bench_decomp1.json
python bench.py --full --workload decomp0 $Q --steps 100 2>/dev/null > $O/bench_decomp0.json
python bench.py --full --workload fst4 $Q --steps 20 --warmup 3 2>/dev/null > $O/bench_fst4.json
python bench.py --full --workload synth512 --batch 1024 --seqlen 128 --steps 3 --warmup 1 $Q --event-stride 1 2>/dev/null > $O/bench_synth512.json
python bench.py --full --workload train --no-cpu-baseline --steps 50 2>/dev/null > $O/bench_train.json
python bench.py --full --workload train --rank 250 --farnn 2 --no-cpu-baseline --steps 20 --warmup 3 2>/dev/null > $O/bench_train_r250_farnn2.json
python bench.py --full --workload train --rank 250 --farnn 2 --batch 1024 --no-cpu-baseline --steps 10 --warmup 2 2>/dev/null > $O/bench_train_r250_farnn2_b1024.json
python scripts/host_inclusive_rate.py 2>/dev/null | grep host-inclusive > $O/host_inclusive.txt
R="--no-cpu-baseline --no-other-configs --no-pipelined --no-parity --event-stride 0"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 bench.py --full --steps 200 --warmup 20 $R > $O/trace.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_s104 -- python3 bench.py --full --workload ifst --states 104 --steps 200 --warmup 20 $R > $O/trace_s104.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_crf -- python3 bench.py --full --workload ifst_crf --steps 100 --warmup 10 $R > $O/trace_crf.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_crf_s104 -- python3 bench.py --full --workload ifst_crf --states 104 --steps 100 --warmup 10 $R > $O/trace_crf_s104.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_decomp -- python3 bench.py --full --workload decomp --steps 100 --warmup 10 $R > $O/trace_decomp.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_decomp_r250 -- python3 bench.py --full --workload decomp --rank 250 --farnn 2 --steps 100 --warmup 10 $R > $O/trace_decomp_r250.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_fst4 -- python3 bench.py --full --workload fst4 --steps 10 --warmup 2 $R > $O/trace_fst4.log 2>&1
P="--steps 20 --warmup 5 $R"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 bench.py --full $P > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 bench.py --full $P > $O/pmc_write.log 2>&1
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/pmc_l2 -- python3 bench.py --full $P > $O/pmc_l2.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_s104 -- python3 bench.py --full --workload ifst --states 104 $P > $O/pmc_fetch_s104.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write_s104 -- python3 bench.py --full --workload ifst --states 104 $P > $O/pmc_write_s104.log 2>&1
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/pmc_l2_s104 -- python3 bench.py --full --workload ifst --states 104 $P > $O/pmc_l2_s104.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_fst4 -- python3 bench.py --full --workload fst4 --steps 3 --warmup 1 $R > $O/pmc_fetch_fst4.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_synth512 -- python3 bench.py --full --workload synth512 --batch 1024 --seqlen 128 --steps 2 --warmup 1 $R > $O/pmc_fetch_synth512.log 2>&1
i=0
for grp in "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_WAIT_ANY" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"; do
  i=$((i+1))
  for wl in ifst decomp ifst_crf; do
    rocprofv3 --pmc $grp --output-format csv -d $O/sq${i}_$wl -- python3 bench.py --full --workload $wl --steps 10 --warmup 3 $R > $O/sq${i}_$wl.log 2>&1
  done
  rocprofv3 --pmc $grp --output-format csv -d $O/sq${i}_ifst104 -- python3 bench.py --full --workload ifst --states 104 --steps 10 --warmup 3 $R > $O/sq${i}_ifst104.log 2>&1
  rocprofv3 --pmc $grp --output-format csv -d $O/sq${i}_rows250 -- python3 bench.py --full --workload decomp --rank 250 --farnn 2 --steps 10 --warmup 3 $R > $O/sq${i}_rows250.log 2>&1
  FARNN_ROWS_LPR4=1 rocprofv3 --pmc $grp --output-format csv -d $O/sq${i}_rows250lpr4 -- python3 bench.py --full --workload decomp --rank 250 --farnn 2 --steps 10 --warmup 3 $R > $O/sq${i}_rows250lpr4.log 2>&1
done
# in-kernel probes (profiling build)
export FARNN_LIB=$PWD/re2nn-seq_amd/csrc/libfarnn_hip_probes.so
Z="--steps 3 --warmup 2 --no-cpu-baseline --no-pipelined --no-other-configs --no-parity"
timeout 120 python bench.py --full $Z 2>/dev/null | grep "^seq" | sort | tail -16 > $O/probe_chain_regs_timeline.txt
FARNN_DBG=1024 timeout 120 python bench.py --full $Z 2>/dev/null | grep "^finish\|^meet" | sort | tail -24 > $O/probe_finish_phases.txt
FARNN_DBG=256 timeout 120 python bench.py --full $Z 2>/dev/null | grep "chain phases" | sort | tail -8 > $O/probe_chain_regs_step_phases.txt
timeout 120 python bench.py --full --workload ifst --states 104 $Z 2>/dev/null | grep "^seq" | sort | tail -16 > $O/probe_chain_wide_s104_timeline.txt
FARNN_DBG=8192 timeout 120 python bench.py --full --workload ifst_crf $Z 2>/dev/null | grep "^viterbi\|^seq" | sort | tail -8 > $O/probe_chain_viterbi_phases.txt
FARNN_DBG=8192 timeout 120 python bench.py --full --workload ifst_crf --states 104 $Z 2>/dev/null | grep "^viterbi\|^seq" | sort | tail -8 > $O/probe_s104_recurrence_then_viterbi_phases.txt
FARNN_DBG=4096 FARNN_NOFUSE=1 timeout 120 python bench.py --full --workload decomp $Z 2>/dev/null | grep "^regs" | sort | tail -4 > $O/probe_decomp_regs8_phases.txt
FARNN_DBG=16 timeout 120 python bench.py --full --workload decomp --rank 250 --farnn 2 --full-length --batch 128 $Z 2>/dev/null | grep "^rows wg" | sort | tail -8 > $O/probe_decomp_rows_r250_step_phases.txt
FARNN_ROWS_LPR4=1 FARNN_DBG=16 timeout 120 python bench.py --full --workload decomp --rank 250 --farnn 2 --full-length --batch 128 $Z 2>/dev/null | grep "^rows wg" | sort | tail -8 > $O/probe_decomp_rows_r250_step_phases_four_lanes_r03.txt
unset FARNN_LIB
# keep only the small summaries (kernel_stats + counter collection), drop per-dispatch traces > 4 MB
find $O -name '*.csv' -size +4M -delete
find $O -name '*kernel_trace.csv' -delete
du -sh $O
