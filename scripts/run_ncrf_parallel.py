#!/usr/bin/env python3
"""Entry point with the reference's program name and arguments (scripts/run_ncrf_parallel.py: --reads, --repeat, -t, -o, --ncrf-bin),
plus --aligner builtin, which writes report.ncrf without any external program; implementation: centroflye_amd/unit_aligner.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.unit_aligner import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
