# Build tools/ab/libsvdj_hip_base.so from a git revision's csrc/hip (block.hip and the
# headers it includes there; default HEAD), linked with the in-tree objects of the
# other HIP sources (A/B runs, SVDJ_HIP_LIB).
set -e
REV=${1:-HEAD}
PK=svd-jacobi-mpi-cuda_amd
T=$(mktemp -d)
git archive $REV $PK/csrc/hip | tar -x -C $T
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$PK/csrc/include -I$T/$PK/csrc/hip \
  -c $T/$PK/csrc/hip/block.hip -o $T/block.o 2>/dev/null
mkdir -p tools/ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $T/block.o \
  $(ls $PK/lib/obj/*.o | grep -v '/block.o$') -o tools/ab/libsvdj_hip_base.so
rm -rf $T
echo "built tools/ab/libsvdj_hip_base.so from $REV"
