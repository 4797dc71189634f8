#!/bin/bash
# Standalone connected_components run without the job server (ETDolphinLauncher
# mode, like run_shortest_path.sh). Multi-GPU: wrap with torchrun (see
# harmony_amd/standalone.py).
cd "$(dirname "$0")/.."
exec python -m harmony_amd.standalone -app connectedcomponents "$@"
