#!/usr/bin/env python3
"""Writes reconstruction_ref.npz in this directory: the inputs of every family and sequence of tests/recon_cases.py and what the
REAL reference's Reconstruction class (oracle/_ref/libvisoref.so, built in place by `make -C oracle ref`) made of them - per
track the stage it ended at, its point, type, distance and angle, and per sequence the tracks every update finished.

    python tests/golden/make_reconstruction_ref.py        # needs the compiled reference; rewrites the .npz

Data only: arrays that the generator and the reference wrote.  tests/test_points_vs_ref.py asserts that the file equals a fresh
run wherever the compiled reference exists; tests/test_points_ref_gpu.py reads it where it does not."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import bindings as B  # noqa: E402
import recon_cases as RC  # noqa: E402

if __name__ == "__main__":
    if not B.have_ref_reconstruction():
        sys.exit("the compiled reference with the Reconstruction entries is missing: make -C oracle ref")
    np.savez_compressed(RC.FIXTURE, **RC.record(B))
    print("wrote", os.path.relpath(RC.FIXTURE, ROOT), os.path.getsize(RC.FIXTURE), "bytes")
