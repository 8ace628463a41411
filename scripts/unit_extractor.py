#!/usr/bin/env python3
"""Entry point beside the reference's script names: the tandem period, the hook k-mer and the unit-length pieces of every raw read
(the reference's scripts/unit_extractor.py, -i -o -k -b); the implementation lives in centroflye_amd/unit_extractor.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.unit_extractor import *  # noqa: E402,F401,F403
from centroflye_amd.unit_extractor import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
