"""numpy reference for the thermal pack (include/mdr.h, mdr_env_bind_thermal_pack): the five columns k01, s0, k10, s1, inv_Ua of
every house as one lossless 128-bit record.  A value is stored as bits(f32) - base_c, base_c the column's smallest bit pattern as
u32, in a field of WIDTHS[c] bits; the fields lie end to end from bit 0, k01 first; plane j of the pack holds dword j of every
house's record.  "Not packed": a column with both signs, with a NaN, or whose largest minus smallest pattern does not fit its field."""
import numpy as np

from mdr_amd import _native as nat

COLUMNS = ("k01", "s0", "k10", "s1", "inv_Ua")
WIDTHS = tuple(nat.MDR_THERMAL_BITS)
OFFSETS = tuple(int(sum(WIDTHS[:c])) for c in range(5))
assert sum(WIDTHS) == 128


def bits(col):
    return np.ascontiguousarray(col, dtype=np.float32).view(np.uint32).ravel()


def thermal_columns(Ua, Cm, Ca, Hm, dt):
    """The five fp32 columns the step kernels read, from fp64 house parameters (csrc/mdr_device.h: thermal_map)."""
    from oracle import mdr_oracle as mo
    m00, m01, m10, m11 = mo.etp_affine_coefficients(np.asarray(Ua, np.float64), np.asarray(Cm, np.float64), np.asarray(Ca, np.float64),
                                                    np.asarray(Hm, np.float64), float(dt))
    cols = (m01, (m00 - 1.0) + m01, m10, m10 + (m11 - 1.0), 1.0 / np.asarray(Ua, np.float64))
    return [np.asarray(c, dtype=np.float32) for c in cols]


def needed_widths(cols):
    """Bits that max - min of each column's patterns takes (a single-valued column: 0)."""
    return tuple(int(int(bits(c).max()) - int(bits(c).min())).bit_length() for c in cols)


def describe(cols):
    """(packed, bases): the descriptor the device writes - words [0] and [1 .. 5]."""
    packed, bases = True, []
    for c, w in zip(cols, WIDTHS):
        b = bits(c)
        lo, hi = int(b.min()), int(b.max())
        bases.append(lo)
        nan = bool(((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)).any())
        mixed = (lo ^ hi) >> 31 != 0
        packed = packed and not nan and not mixed and hi - lo < (1 << w)
    return packed, np.array(bases, dtype=np.uint32)


def pack(cols):
    """(packed, bases, planes uint32 [4][n]); planes is None when not packed."""
    packed, bases = describe(cols)
    if not packed:
        return False, bases, None
    n = bits(cols[0]).size
    fields = [(bits(c) - bases[i]).astype(np.uint64) for i, c in enumerate(cols)]
    lo = np.zeros(n, dtype=np.uint64)              # record bits 0 .. 63
    hi = np.zeros(n, dtype=np.uint64)              # record bits 64 .. 127
    for f, off, w in zip(fields, OFFSETS, WIDTHS):
        assert int(f.max()) < (1 << w)
        if off < 64:
            lo |= f << np.uint64(off)              # (bits shifted past 63 drop off: they are added to `hi` below)
            if off + w > 64:
                hi |= f >> np.uint64(64 - off)
        else:
            hi |= f << np.uint64(off - 64)
    m32 = np.uint64(0xFFFFFFFF)
    planes = np.stack([(lo & m32), (lo >> np.uint64(32)), (hi & m32), (hi >> np.uint64(32))]).astype(np.uint32)
    return True, bases, planes


def fields(planes):
    """The five raw fields (uint32, flat) of every record."""
    p = planes.astype(np.uint64)
    lo = p[0] | (p[1] << np.uint64(32))
    hi = p[2] | (p[3] << np.uint64(32))
    out = []
    for off, w in zip(OFFSETS, WIDTHS):
        mask = np.uint64((1 << w) - 1)
        if off + w <= 64:
            f = (lo >> np.uint64(off)) & mask
        elif off >= 64:
            f = (hi >> np.uint64(off - 64)) & mask
        else:
            f = ((lo >> np.uint64(off)) | (hi << np.uint64(64 - off))) & mask
        out.append(f.astype(np.uint32))
    return out


def unpack(bases, planes):
    """The five fp32 columns (flat) back from the records."""
    return [(f + np.uint32(bases[c])).view(np.float32) for c, f in enumerate(fields(planes))]
