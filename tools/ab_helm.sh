set -o pipefail
O=${O:-out/ab_helm}; mkdir -p $O
for r in 1 2; do for v in base rmw; do lib=""; [ $v != base ] && lib=ablib/$v/libslu_mi355x.so
SLU_LIB=$lib timeout -k 10 400 python -u bench.py --full --workload helm3d --steps 3 --warmup 1 --no-next --no-abi > $O/h_$v.json 2>/dev/null || exit 1
python -c "import json; d=json.load(open('$O/h_$v.json')); r=d['roofline']; print('helm3d $v', d['ms_per_step'], r['frac'], r['serial_factor_ms'])"; done; done
