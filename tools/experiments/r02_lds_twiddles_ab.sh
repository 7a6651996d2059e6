O=${1:?usage: r02_lds_twiddles_ab.sh OUTDIR [UBENCH binary]}; UB=${2:-./ubench}; mkdir -p $O
timeout 120 $UB 3 > $O/ubench.txt 2>&1; grep -h "ABL=  0 \|ABL= 56\|ABL= 48\|ABL= 64" $O/ubench.txt
timeout 200 python -m pytest tests -m gpu -x -q --timeout 300 -k "tuned or config3 or big_batches" 2>&1 | tail -2
for i in 1 2; do timeout 100 python bench.py --full --no-cpu --streams 1 > $O/bench_s1_$i.json 2>> $O/err; done
timeout 100 python bench.py --full --no-cpu > $O/bench_s2.json 2>> $O/err
python - $O <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + '/bench_*.json')):
    d=json.loads(open(f).read().strip().splitlines()[-1]); r=d['roofline']
    print(f.split('/')[-1], 'value %.1f'%d['value'], 'dev_us %.2f'%r['device_us_per_step'], 'pass', r.get('pass_us'), d.get('verified'))
PY
