"""Builds tests/golden/ticks_bid_8x2049.npz from VectorWave's ES tick archive.

Run by hand on a machine that has the reference checkout (never by a test):

    python tests/golden/make_tick_fixture.py <reference>/vectorwave-core/src/test/resources/ticks_1734964200000L.tar.xz

The archive holds one CSV of `timestamp,side,size,price` rows.  The fixture is the price of the first
8 * 2049 rows whose side is BID, in file order, as 8 rows of 2049 float64 (array name `prices`): real tick
prices, quantised to 0.25, so most level-1 detail coefficients of a row's returns are exactly 0.0.
Standard library only (tarfile / lzma read the archive, zipfile writes the .npz by hand).
"""
import os
import struct
import sys
import tarfile
import zipfile

ROWS, COLS = 8, 2049
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ticks_bid_8x2049.npz")


def bid_prices(archive: str, count: int):
    out = []
    with tarfile.open(archive, "r:xz") as tar:
        member = next(m for m in tar.getmembers() if m.isfile())
        with tar.extractfile(member) as f:
            for line in f:
                fields = line.decode("ascii").strip().split(",")
                if len(fields) >= 4 and fields[1] == "BID":
                    out.append(float(fields[3]))
                    if len(out) == count:
                        break
    if len(out) != count:
        raise SystemExit(f"only {len(out)} BID rows in {archive}")
    return out


def npy_bytes(values, shape) -> bytes:
    """NPY format 1.0: magic, version, little-endian header length, dict padded so the data starts at a multiple of 64."""
    header = "{'descr': '<f8', 'fortran_order': False, 'shape': (%d, %d), }" % shape
    pad = 64 - (10 + len(header) + 1) % 64
    header = header + " " * (pad % 64) + "\n"
    return b"\x93NUMPY\x01\x00" + struct.pack("<H", len(header)) + header.encode("latin1") + \
        struct.pack("<%dd" % len(values), *values)


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__)
        return 2
    prices = bid_prices(argv[1], ROWS * COLS)
    info = zipfile.ZipInfo("prices.npy", date_time=(1980, 1, 1, 0, 0, 0))  # fixed stamp: reproducible bytes
    info.compress_type = zipfile.ZIP_DEFLATED
    with zipfile.ZipFile(OUT, "w") as z:
        z.writestr(info, npy_bytes(prices, (ROWS, COLS)), compresslevel=9)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(set(prices))} distinct prices, "
          f"{min(prices)}..{max(prices)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
