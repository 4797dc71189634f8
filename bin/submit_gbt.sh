#!/bin/bash
# Submit a gbt job to the running job server (reference submit_gbt.sh flags).
# -test_data_path <file> (with or without file://): a held-out file in the
# -input format, read whole by every rank before training; the summary then
# holds test_mse or test_error_rate and test_examples.
cd "$(dirname "$0")/.."
exec python -m harmony_amd.jobserver.client submit -app gbt "$@"
