#!/usr/bin/env python3
"""Flat-import shim: the reference's scripts import their siblings as `from mono_error_correction import ...`.
Implementation: centroflye_amd/mono_error_correction.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from centroflye_amd.mono_error_correction import *  # noqa: E402,F401,F403
