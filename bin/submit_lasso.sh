#!/bin/bash
# Submit a lasso job to the running job server (reference submit_lasso.sh flags).
# -test_data_path <file> (with or without file://): a held-out file in the
# -input format, read whole by every rank before training; the summary then
# holds test_mse and test_examples.
cd "$(dirname "$0")/.."
exec python -m harmony_amd.jobserver.client submit -app lasso "$@"
