"""Writes tests/golden/shapefiles/: the whole records of a Natural Earth countries.shp and lakes.shp (the set the
reference ships under res/shapefiles/) whose bounding boxes meet South America.

    python tools/make_map_fixture.py SHAPEFILE_DIR

Records are copied byte for byte and renumbered; the header's file length and bounding box are rewritten."""
import os
import struct
import sys

BOX = (-95.0, -60.0, -25.0, 15.0)  # lon min, lat min, lon max, lat max
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "shapefiles")


def clip(src, dst):
    with open(src, "rb") as f:
        data = f.read()
    header = bytearray(data[:100])
    pos, out, n = 100, [], 0
    bbox = [float("inf"), float("inf"), -float("inf"), -float("inf")]
    while pos + 8 <= len(data):
        length = struct.unpack(">i", data[pos + 4:pos + 8])[0] * 2
        body = data[pos + 8:pos + 8 + length]
        pos += 8 + length
        if struct.unpack("<i", body[:4])[0] == 0:
            continue
        xmin, ymin, xmax, ymax = struct.unpack("<4d", body[4:36])
        if xmax < BOX[0] or xmin > BOX[2] or ymax < BOX[1] or ymin > BOX[3]:
            continue
        n += 1
        out.append(struct.pack(">ii", n, length // 2) + body)
        bbox = [min(bbox[0], xmin), min(bbox[1], ymin), max(bbox[2], xmax), max(bbox[3], ymax)]
    blob = b"".join(out)
    header[24:28] = struct.pack(">i", (100 + len(blob)) // 2)
    header[36:68] = struct.pack("<4d", *bbox)
    with open(dst, "wb") as f:
        f.write(bytes(header) + blob)
    print(f"{dst}: {n} records, {100 + len(blob)} bytes")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    os.makedirs(OUT, exist_ok=True)
    for name in ("countries.shp", "lakes.shp"):
        clip(os.path.join(sys.argv[1], name), os.path.join(OUT, name))


if __name__ == "__main__":
    main()
