# Same-box A/B of two builds of the library (GPU boxes differ by a few percent, so variants are compared inside one
# gpurun call):  python vic_amd/build.py -f -o vic_amd/libvicgpu_b.so -DVARIANT ; gpurun -- 'bash tools/ab.sh'
# B_DIR=dir: run side b's bench.py from a checkout of the commit libvicgpu_b.so was built from (needed when that commit's
# Python layer declares other entry points than this one's).  REPS=n: repetitions per side (default 2).  MASK_LINE=1: one
# more run of library a with a retire mask set on every context and no failing cell (tools/ab_mask.py): what the kernels'
# validity-table loads cost.
ROOT=$PWD
ARGS=${BENCH_ARGS:---config cfg3 --steps 4 --warmup 1 --no-cpu-baseline}
line() { python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$1 ms_per_step %.2f' % d['ms_per_step'])"; }
for rep in $(seq 1 ${REPS:-2}); do
  for v in a b; do
    lib=vic_amd/libvicgpu.so; dir=.; [ $v = b ] && { lib=vic_amd/libvicgpu_b.so; dir=${B_DIR:-.}; }
    (cd $dir && VICGPU_LIB=$ROOT/$lib timeout -k 10 300 python bench.py $ARGS 2>/dev/null) | line "$v rep$rep" || exit 1
  done
done
if [ -n "${MASK_LINE:-}" ]; then
  VICGPU_LIB=$PWD/vic_amd/libvicgpu.so timeout -k 10 300 python tools/ab_mask.py $ARGS 2>/dev/null | line "a mask" || exit 1
fi
