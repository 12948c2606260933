# chain streams x run-ahead for the GPU-resident form, interleaved on one box
run() { echo -n "$1: "; timeout -k 5 120 python bench.py --full --no-cpu-baseline --no-per-frame --no-alone --no-verify --steps ${STEPS:-20} --warmup 3 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); s=sorted(d['step_ms_rank0']); print(d['value'], d['ms_per_step'], 'min %.2f median %.2f max %.2f' % (s[0], s[len(s)//2], s[-1]))"; }
export VSM_HOST_THREADS=${T:-16}
for rep in 1 2; do for n in 2 3 4; do VSM_SEQ_DC_STREAMS=$n run "dc streams=$n" || exit 1; done; done
