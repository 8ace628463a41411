#!/usr/bin/env python3
"""Flat-import shim and entry point: the reference's scripts import their siblings as `from sd_parser import ...`; -i REPORT -m MONOMERS
prints the statistics of the report's monostrings.  Implementation: centroflye_amd/sd_parser.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.sd_parser import *  # noqa: E402,F401,F403
from centroflye_amd.sd_parser import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
