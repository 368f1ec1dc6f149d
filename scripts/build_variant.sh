#!/bin/bash
# Builds casualhdrsplat_amd/libhdrsplat_<name>.so = the product sources with extra -D flags on some translation units (A/B
# and ablation experiments): `make variant` of casualhdrsplat_amd/csrc/Makefile under its older command line.
# usage: bash scripts/build_variant.sh <name> <tu[,tu...]: any unit of the Makefile's OBJS, e.g. binning,render> "<flags>"
set -e
make -s -C "$(dirname "$0")/../casualhdrsplat_amd/csrc" variant NAME="$1" TUS="${2//,/ }" DEFS="$3"
echo "built casualhdrsplat_amd/libhdrsplat_$1.so"
