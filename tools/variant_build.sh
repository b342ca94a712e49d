#!/bin/bash
# Build an experimental variant of the library next to the product one, for in-process A/B timing with tools/ab_lib.py:
#   tools/variant_build.sh NAME "-DMACRO=1 ..."   ->  directx-raytracer_amd/libcrt_hip_NAME.so
# The five traversal units (render_kernels.hip, path_kernels.hip, ray_kernels.hip, point_kernels.hip, list_kernels.hip) and the
# host units of the C-ABI layer (crt_api.cpp and the api_*.cpp beside it) are recompiled with the extra flags; every other object
# of the Makefile's list is shared with the product build.
set -e
NAME=$1; FLAGS=$2; HIPONLY=$3   # optional third argument: flags for hipcc only (e.g. "-mllvm -option")
cd "$(dirname "$0")/../directx-raytracer_amd/csrc"
make -j8 > /dev/null
UNITS="render_kernels path_kernels ray_kernels point_kernels list_kernels"
HOST="crt_api api_frames api_queries api_image api_dynamic api_comm api_scene"
for u in $UNITS; do
    /opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC -ffp-contract=off -fno-fast-math --offload-arch=gfx950 $FLAGS $HIPONLY -c $u.hip -o build/${u}_$NAME.o &
done
for u in $HOST; do
    g++ -std=c++17 -O3 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $FLAGS -c $u.cpp -o build/${u}_$NAME.o &
done
wait
# the Makefile's object list, with the recompiled units in place of the product's
OBJ=$(make -pn | sed -n 's/^OBJ = //p' | head -1)
for u in $UNITS $HOST; do OBJ=${OBJ/build\/$u.o/build\/${u}_$NAME.o}; done
g++ -shared -o ../libcrt_hip_$NAME.so $OBJ -Wl,--version-script=exports.map -L/opt/rocm/lib -lamdhip64 -ldl -fopenmp -Wl,-rpath,/opt/rocm/lib
for u in $UNITS $HOST; do rm -f build/${u}_$NAME.o; done
echo "built directx-raytracer_amd/libcrt_hip_$NAME.so"
