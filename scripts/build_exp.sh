#!/bin/bash
# Experiment build: lib/libmi3dsparse_exp.so (`make exp`; EXP_FLAGS adds further -D switches).
set -e
make -j"${JOBS:-8}" -C "$(dirname "$0")/../3d-weakly-supervised-semantic-segmentation_amd/csrc" exp EXP_FLAGS="${EXP_FLAGS:-}"
