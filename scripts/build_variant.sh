#!/bin/bash
# build_variant.sh <name> [-DFLAG ...]: a build of the library with extra flags, as variants/<name>.so
# (no GPU needed; for A/B runs with TURTLE_AMD_LIBRARY).  The flags go to ONE unit of the device layer,
# device.hip unless UNIT= names another (UNIT=rays: rays.hip); SRC= another copy of that unit.  The
# other units, the thread runtime (runtime.hip) and the host objects are the tree's own, as make built them
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
unit=${UNIT:-device}
mkdir -p $ROOT/variants $ROOT/turtle_amd/csrc/build
make -s -C $ROOT/turtle_amd/csrc >/dev/null
obj=$ROOT/turtle_amd/csrc/build/${unit}_$name.o
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 -I$ROOT/include -I$ROOT/turtle_amd/csrc "$@" \
    -c ${SRC:-$ROOT/turtle_amd/csrc/$unit.hip} -o $obj
# (the unit being replaced and every variant of any unit, <unit>_<name>.o, stay out: no source file has a _ in its name)
others=$(ls $ROOT/turtle_amd/csrc/build/*.o | grep -v -e "/$unit\.o$" -e "/[a-z]*_[^/]*\.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $ROOT/variants/$name.so $others $obj -lm -lz
echo $ROOT/variants/$name.so
