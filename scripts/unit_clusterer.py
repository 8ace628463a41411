#!/usr/bin/env python3
"""Entry point beside the reference's script names: the consensus length class of many reads' units and its median unit (the
reference's scripts/unit_clusterer.py, -i -o -b); the implementation lives in centroflye_amd/unit_clusterer.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.unit_clusterer import *  # noqa: E402,F401,F403
from centroflye_amd.unit_clusterer import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
