#!/bin/bash
# Submit a mlr job to the running job server (reference submit_mlr.sh flags).
# -test_data_path <file> (with or without file://): a held-out file in the
# -input format, read whole by every rank before training; the summary then
# holds test_cross_entropy, test_accuracy and test_examples.
cd "$(dirname "$0")/.."
exec python -m harmony_amd.jobserver.client submit -app mlr "$@"
