#!/usr/bin/env python3
"""Entry point beside the reference's script names: map reads onto the contig of a finished read_positions.csv
(the reference's cloud_contig.map_reads_fast, which no script of its own calls; --exact, --check-exact and --rescore-placed
ask its exact scorer, calc_inters_score / map_reads, as well); the implementation lives in centroflye_amd/read_mapper.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.read_mapper import *  # noqa: E402,F401,F403
from centroflye_amd.read_mapper import main  # noqa: E402

if __name__ == "__main__":
    main()
