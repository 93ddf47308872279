#!/bin/bash
# One command to re-establish everything this repository claims.
#   here (no GPU):     tools/validate_all.sh cpu      build (hipcc cross-compiles gfx950) + CPU tests
#   on an MI355X box:  tools/validate_all.sh gpu      GPU parity tests + smoke + default bench line
#                      tools/validate_all.sh profile <tag>   rocprofv3 kernel stats + PMC passes -> gpurun_out/prof_<tag>/
#                                                    (then, back in the build container: python tools/summarize_round.py <tag>)
# A failing step stops the script (no further GPU step is started after a failure).
set -euo pipefail
cd "$(dirname "$0")/.."
case "${1:-cpu}" in
  cpu)
    python __graft_entry__.py
    python -m pytest tests -x -q -m "not gpu"
    # the volume unit alone: restatement, compiled core (also under the sanitizers), ABI
    python -m pytest tests/test_mesh_volume_ref.py tests/test_volume_core_cpu.py tests/test_volume_device_abi.py -q
    # the mesh-to-mesh distance alone: restatement, compiled core (also under the sanitizers), ABI
    python -m pytest tests/test_mesh_proximity_ref.py tests/test_proximity_core_cpu.py tests/test_proximity_device_abi.py -q
    # the localization mapping alone: restatement, compiled core (also under the sanitizers), ABI
    python -m pytest tests/test_surface_mapping_ref.py tests/test_mapping_core_cpu.py tests/test_mapping_device_abi.py -q
    # DBSCAN clustering alone: restatement (against scikit-learn), compiled core (also under the sanitizers), ABI
    python -m pytest tests/test_dbscan_ref.py tests/test_clustering_core_cpu.py tests/test_clustering_device_abi.py -q
    ;;
  gpu)
    timeout -k 10 900 python -m pytest tests -x -q -m gpu
    python -c "import __graft_entry__ as g; g.smoke()"
    python bench.py
    timeout -k 10 600 python tools/volume_profile.py c3
    timeout -k 10 600 python tools/proximity_profile.py
    timeout -k 10 600 python tools/mapping_profile.py
    timeout -k 10 600 python tools/clustering_profile.py c3 1.0
    ;;
  profile)
    tools/profile_round.sh "${2:?tag}"
    ;;
  *)
    echo "usage: $0 cpu|gpu|profile <tag>"; exit 2;;
esac
