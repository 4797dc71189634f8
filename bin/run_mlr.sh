#!/bin/bash
# Standalone mlr run without the job server (reference run_mlr.sh /
# ETDolphinLauncher mode). Multi-GPU: wrap with torchrun (see
# harmony_amd/standalone.py).
# -test_data_path <file> (with or without file://): a held-out file in the
# -input format, read whole by every rank before training; the summary then
# holds test_cross_entropy, test_accuracy and test_examples.
cd "$(dirname "$0")/.."
exec python -m harmony_amd.standalone -app mlr "$@"
