"""One rank process of an IPC world running the block moves with irregular datatypes, started by
tests/test_gpu_indexed_ipc.py.

    python tests/indexed_ipc_worker.py RANK P UID_HEX BASE

tests/strided_ipc_worker.py with the cases replaced by tests/indexed_cases.py: the same JSON line.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import indexed_cases  # noqa: E402
import strided_ipc_worker  # noqa: E402

if __name__ == "__main__":
    strided_ipc_worker.SC = indexed_cases
    sys.exit(strided_ipc_worker.main())
