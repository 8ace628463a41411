#!/usr/bin/env python3
"""Entry point with the reference's script name and CLI (centroFlye.py:212-225 calls
`python -u scripts/better_consensus_unit_reconstruction.py ...`); the implementation lives in centroflye_amd/better_consensus_unit_reconstruction.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.better_consensus_unit_reconstruction import *  # noqa: E402,F401,F403
from centroflye_amd.better_consensus_unit_reconstruction import main  # noqa: E402

if __name__ == "__main__":
    main()
