"""The mailbox step and halo entry points (mdr_env_step_mailbox, mdr_mailbox_halo_*) are exported and validate their arguments
without touching the GPU; sharding.MailboxExchange imports and checks its timeout.  No GPU here."""
import ctypes as C

import pytest

import mdr_amd
from mdr_amd import _native as nat


def _lib():
    mdr_amd.build_native()
    return mdr_amd.load_native()


def test_mailbox_step_and_halo_are_exported():
    lib = _lib()
    for name in ("mdr_env_step_mailbox", "mdr_mailbox_halo_bytes", "mdr_mailbox_halo_push", "mdr_mailbox_halo_pull"):
        assert name in nat.EXPORTS and hasattr(lib, name), name
    assert lib.mdr_mailbox_halo_bytes(2, 1000) == 2 * 2 * 1000 * 8      # two slots x world x count granules of 8 bytes
    assert lib.mdr_mailbox_halo_bytes(0, 1000) == 0 and lib.mdr_mailbox_halo_bytes(nat.MDR_MAX_SHARDS + 1, 1) == 0


def test_null_env_or_bad_mailbox_is_refused_without_the_gpu():
    lib = _lib()
    mb = nat.MdrMailbox()                      # struct_size 0
    assert lib.mdr_env_step_mailbox(None, None, nat.ACTIONS_EXTERNAL, C.byref(mb), 0, None) == nat.MDR_ERR_INVALID
    cfg = nat.MdrConfig()                      # invalid config: create returns a handle that explains, no device work
    h = C.c_void_p()
    assert lib.mdr_env_create(C.byref(cfg), C.byref(h)) == nat.MDR_ERR_INVALID
    try:
        assert lib.mdr_env_step_mailbox(h, None, nat.ACTIONS_EXTERNAL, C.byref(mb), 0, None) == nat.MDR_ERR_INVALID
        assert b"size mismatch" in lib.mdr_last_error(h)
        assert lib.mdr_env_step_mailbox(h, None, nat.ACTIONS_EXTERNAL, None, 0, None) == nat.MDR_ERR_INVALID
    finally:
        lib.mdr_env_destroy(h)
    buf = (C.c_float * 4)()
    assert lib.mdr_mailbox_halo_push(C.byref(mb), 1, buf, 4, 1, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_mailbox_halo_pull(C.byref(mb), 1, buf, 4, 1, 0, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_mailbox_halo_push(None, 1, buf, 4, 1, None) == nat.MDR_ERR_INVALID
    assert lib.mdr_mailbox_halo_pull(None, 1, buf, 4, 1, 0, None) == nat.MDR_ERR_INVALID


def test_mailbox_exchange_imports_and_checks_its_timeout():
    from mdr_amd.sharding import MailboxExchange, TorchDistExchange
    ex = MailboxExchange(timeout_ms=3)
    assert isinstance(ex, TorchDistExchange)
    assert ex.timeout_us == 3000 and ex.capturable is False
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError):
            MailboxExchange(timeout_ms=bad)
