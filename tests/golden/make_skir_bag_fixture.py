"""Writes tests/golden/skir_voxel_map.bag.xz: the reference's skir.bag (mpl_test_node/maps/skir/skir.bag) cut down to
its /voxel_map topic, so that tests/test_rosbag_io.py reads a real bag without the reference tree.

    python tests/golden/make_skir_bag_fixture.py <path of skir.bag>

The bag-header record and the /voxel_map connection and message records are copied byte for byte; they are put into
one uncompressed chunk, as in the original.  The /cloud topic (a 3.5 MB point cloud no test reads), its connection and
the index records are left out.  The result is xz-compressed.
"""
import lzma
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from mpl_ros_amd import rosbag_io  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skir_voxel_map.bag.xz")
MAGIC = b"#ROSBAG V2.0\n"


def _raw_records(buf, i=0):
    """(header fields, the record's bytes) in file order"""
    while i + 8 <= len(buf):
        (hl,) = struct.unpack_from("<I", buf, i)
        (dl,) = struct.unpack_from("<I", buf, i + 4 + hl)
        yield rosbag_io._fields(buf[i + 4:i + 4 + hl]), buf[i:i + 8 + hl + dl], buf[i + 8 + hl:i + 8 + hl + dl]
        i += 8 + hl + dl


def main(bag):
    buf = open(bag, "rb").read()
    assert buf.startswith(MAGIC)
    out, inner = MAGIC, b""
    for hdr, rec, data in _raw_records(buf, len(MAGIC)):
        op = hdr["op"][0]
        if op == rosbag_io.OP_BAG_HEADER:
            out += rec
        elif op == rosbag_io.OP_CHUNK:
            assert hdr.get("compression", b"none") == b"none"
            for h, r, _ in _raw_records(data):
                if h["op"][0] in (rosbag_io.OP_CONNECTION, rosbag_io.OP_MSG) and struct.unpack("<I", h["conn"])[0] == 0:
                    inner += r
    topics = {cid: t for cid, (t, _) in rosbag_io.read_messages(bag)[0].items()}
    assert topics[0] == "/voxel_map" and inner
    chunk_hdr = b"".join(struct.pack("<I", len(f)) + f for f in (b"compression=none", b"op=" + bytes([rosbag_io.OP_CHUNK]),
                                                                   b"size=" + struct.pack("<I", len(inner))))
    out += struct.pack("<I", len(chunk_hdr)) + chunk_hdr + struct.pack("<I", len(inner)) + inner
    with open(OUT, "wb") as f:
        f.write(lzma.compress(out, preset=9 | lzma.PRESET_EXTREME))
    print("wrote", OUT, os.path.getsize(OUT), "bytes (bag of", len(out), "bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
