#!/bin/bash
# usage: scratch/build_variant.sh <name> "<extra hipcc flags>"  -> scratch/variants/<name>.so (a libmdbg_hip.so built with the flags)
# MDBG_SRC=<another checkout's rust_mdbg_amd/csrc>: libmdbg.hip is compiled from there (an A/B against a parent commit); the graph stages' objects are this tree's.
# On the GPU box: cp scratch/variants/<name>.so rust_mdbg_amd/libmdbg_hip.so  (the box's copy of the repo is scratch)
set -e
N=$1; shift
D=$(cd $(dirname $0)/.. && pwd)
mkdir -p $D/scratch/variants /tmp/variant_$N
cd ${MDBG_SRC:-$D/rust_mdbg_amd/csrc}
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function "$@" -c -o /tmp/variant_$N/libmdbg.o libmdbg.hip
cd $D/rust_mdbg_amd/csrc
OBJ="edges.o unitigs.o simplify.o components.o contigs.o node_seqs.o placement.o read_paths.o junctions.o transits.o repeats.o superbubbles.o"      # Makefile: OBJ without libmdbg.o
make $OBJ
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o $D/scratch/variants/$N.so /tmp/variant_$N/libmdbg.o $OBJ -ldl
ls -la $D/scratch/variants/$N.so
