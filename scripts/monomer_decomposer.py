#!/usr/bin/env python3
"""Entry point of the built-in monomer decomposer: -s/--sequences READS -m/--monomers FASTA [-o decomposition.tsv] [--match --mismatch
--gap --min-identity] [-t N]; writes the six-column report scripts/sd_parser.py reads.  It is NOT String Decomposer;
implementation: centroflye_amd/monomer_decomposer.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.monomer_decomposer import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
