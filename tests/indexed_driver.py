"""Runs the irregular datatypes' method matrix (tests/indexed_cases.py) on rank threads in a fresh process.

    python tests/indexed_driver.py smp|rccl P[,P...] BASE[,BASE...]

tests/strided_driver.py with the cases replaced: the same worlds, the same JSON line.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import indexed_cases  # noqa: E402
import strided_driver  # noqa: E402

if __name__ == "__main__":
    strided_driver.SC = indexed_cases
    sys.exit(strided_driver.main())
