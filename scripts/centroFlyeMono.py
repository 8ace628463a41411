#!/usr/bin/env python3
"""Entry point of the cen6 pipeline up to the polished scaffolds (--stop-after correction | graph | mapping | scaffolds | pseudounits | polishing).  Implementation: centroflye_amd/centroflye_mono.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.centroflye_mono import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
