"""The reference of the string-range suites (test_gpu_str_range*.py, test_str_range_host.py): IMM3_STR_RANGE restated over Python
`bytes` objects, whose comparison IS unsigned lexicographic byte order, plus the data the byte-order cases are built from."""
import numpy as np


def pad(lo, hi, width):
    """the ABI's padding: lo with 0x00, hi with 0xFF, to the column's width"""
    return bytes(lo) + b"\x00" * (width - len(lo)), bytes(hi) + b"\xff" * (width - len(hi))


def in_range(rows, lo, hi):
    """bool[n]: lo' <= row <= hi' for the rows of a uint8[n, width] array"""
    rows = np.asarray(rows, dtype=np.uint8)
    n, width = rows.shape
    plo, phi = pad(lo, hi, width)
    return np.fromiter((plo <= r.tobytes() <= phi for r in rows), dtype=bool, count=n)


def bitmap_words(mask, block_rows):
    """the batch-major bitmap of a row mask: ceil(rows / 64) uint64 words per block, bit i of a block = word i >> 6, bit i & 63"""
    out, pos = [], 0
    for n in block_rows:
        bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
        bits[:n] = mask[pos:pos + n]
        out.append(np.packbits(bits, bitorder="little").view("<u8"))
        pos += n
    return np.concatenate(out) if out else np.zeros(0, dtype="<u8")


def successor(v):
    """the next value of len(v) bytes in byte order, or None behind FF .. FF"""
    n = int.from_bytes(v, "big") + 1
    return None if n >> (8 * len(v)) else n.to_bytes(len(v), "big")


def predecessor(v):
    n = int.from_bytes(v, "big")
    return None if n == 0 else (n - 1).to_bytes(len(v), "big")


def byte_positions(width):
    """every byte of the row up to width 20; above: the ends of the first dword, of the 16-byte prefix, the first tail bytes, the last"""
    return list(range(width)) if width <= 20 else sorted({0, 3, 4, 15, 16, 17, width - 1})


def neighbours(bound, width):
    """Rows around a full-width bound: the bound itself, its predecessor and successor (carries included), and for every byte position
    of byte_positions rows that differ from the bound in that byte alone -- by 0x7F / 0x80 (a signed compare orders them the other way
    round) and by 0x00 / 0xFF."""
    rows = [bound]
    for nb in (predecessor(bound), successor(bound)):
        if nb is not None:
            rows.append(nb)
    for b in byte_positions(width):
        for x in (0x00, 0x7F, 0x80, 0xFF, (bound[b] + 1) & 0xFF, (bound[b] - 1) & 0xFF):
            rows.append(bound[:b] + bytes([x]) + bound[b + 1:])
    return rows


def carry_bounds(width):
    """bounds whose predecessor / successor carry across dword boundaries: .. 00 FF FF FF FF and .. 01 00 00 00 00 (as far as the
    width allows), and the all-00 / all-FF ends"""
    out = [b"\x00" * width, b"\xff" * width]
    if width >= 2:
        k = min(4, width - 1)
        out.append(b"m" * (width - k - 1) + b"\x00" + b"\xff" * k)
        out.append(b"m" * (width - k - 1) + b"\x01" + b"\x00" * k)
    return out


def rows_array(rows, width):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, width).copy()
