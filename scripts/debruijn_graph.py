#!/usr/bin/env python3
"""Flat-import shim: the reference's scripts import their siblings as `from debruijn_graph import ...`.
Implementation: centroflye_amd/debruijn_graph.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.debruijn_graph import *  # noqa: E402,F401,F403
