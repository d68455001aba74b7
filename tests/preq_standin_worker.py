"""Child process of tests/test_gpu_preq.py: persistent requests in a world that is not a direct multicore world.
Two rank threads form an "RCCL" world over the stand-in build (tests/rccl_standin_driver.py loads it and makes
the world); mpjx_send_init and mpjx_recv_init must return MPJX_ERR_UNSUPPORTED there, as mpjx_isend does, and
leave the handle NULL. Prints PREQ STANDIN OK."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rccl_standin_driver as D  # noqa: E402  (selects the stand-in library before the package loads one)

MPJX_ERR_UNSUPPORTED = -6


def main():
    L = D.L
    comms = D.world(2)

    def body(r):
        c = comms[r]
        buf = D.torch.zeros(4, dtype=D.torch.int32, device="cuda")
        h = ctypes.c_void_p()
        codes = [L.mpjx_send_init(c.handle, buf.data_ptr(), 4, 5, 1 - r, 0, ctypes.byref(h)), bool(h.value),
                 L.mpjx_recv_init(c.handle, buf.data_ptr(), 4, 5, 1 - r, 0, ctypes.byref(h)), bool(h.value),
                 L.mpjx_isend(c.handle, buf.data_ptr(), 4, 5, 1 - r, 0, ctypes.byref(h)), bool(h.value),
                 L.mpjx_comm_p2p_pool_stats(c.handle, None, None, None, None, None)]
        try:
            c.Send_init(buf, 0, 4, D.MPI.INT, 1 - r, 0)
            codes.append("returned")
        except D.mpi.MPIException as e:
            codes.append("(-6)" in str(e) and "multicore worlds" in str(e))
        return codes
    out = D.threads(2, body)
    D.free(comms)
    want = [MPJX_ERR_UNSUPPORTED, False] * 3 + [MPJX_ERR_UNSUPPORTED, True]
    assert out == [want, want], out
    print("PREQ STANDIN OK")


if __name__ == "__main__":
    main()
