cd $GRAFT_REPO_ROOT
pr() { python -c "import sys,json; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$1 tok/s %.3g ms/step %.4f chain_us %.1f frac %.3f achieved %.0f GB/s score_us %.1f' % (d['value'], d['ms_per_step'], r['kernel_avg_us'], r['frac'], r['achieved'], r['score_decode_avg_us']))"; }
E=$(mktemp)                                                        # each run's stderr, for its last lines
python bench.py --full --workload synth512 --batch 256 --seqlen 64 --steps 5 --warmup 2 --no-cpu-baseline --event-stride 1 2>$E | pr "synth512 B256 L64"
tail -3 $E
python bench.py --full --workload synth512 --batch 1024 --seqlen 128 --steps 3 --warmup 1 --no-cpu-baseline --event-stride 1 2>$E | pr "synth512 B1024 L128"
tail -3 $E
rm -f $E
