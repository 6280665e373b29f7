#!/usr/bin/env python3
"""Generates cudadepthmapintegration_amd/csrc/isosurface_table.inc: the marching-cubes case table of csrc/isosurface.hip.

The table is derived from one rule, not typed in:
  * corner c of a cell is at (c & 1, (c >> 1) & 1, c >> 2); bit c of the case index is set when corner c is inside;
  * an edge is crossed when exactly one of its two corners is inside;
  * on each of the six cube faces the crossed edges (0, 2 or 4 of them) are paired into segments; on an ambiguous face
    (two diagonal inside corners, four crossed edges) each inside corner's two crossed edges form a segment, i.e. the
    inside corners are separated;
  * a segment p -> q on a face is directed so that the face's inside corners lie to the left of it seen from outside
    the cube, which makes the loops run counter-clockwise around the outward normal of the surface; every crossed edge
    is in exactly two segments (one per face it lies on), so the segments form closed loops;
  * loops are taken in the order of their lowest edge; each is fan-triangulated from its first edge, the lowest of its
    edges from which no diagonal of the fan joins two edges of one cube face (such a diagonal lies in the face, and the
    cell on its other side may draw the same one: four triangles on one mesh edge).
The face rule depends on the face's four corners alone, so two cells sharing a face draw the same segments there (in
opposite directions): the surface is closed and consistently oriented by construction.

Importable: tests/isosurface_np.py reads EDGES / TRI_COUNT / TRIS from here, the kernel from the generated file.
"""
import os

# Edge e: (axis, offset of its lower corner).  Edges 0-3 run along x, 4-7 along y, 8-11 along z; within an axis the two
# other coordinates count up, the first one fastest.
EDGES = []
for _d in range(3):
    _o1, _o2 = [a for a in range(3) if a != _d]
    for _b in range(4):
        _off = [0, 0, 0]
        _off[_o1], _off[_o2] = _b & 1, _b >> 1
        EDGES.append((_d, tuple(_off)))


def _corner(off):
    return off[0] + 2 * off[1] + 4 * off[2]


def edge_corners(e):
    d, off = EDGES[e]
    b = list(off)
    b[d] = 1
    return _corner(off), _corner(b)


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, c >> 2)


def edge_mid(e):
    a, b = edge_corners(e)
    pa, pb = corner_pos(a), corner_pos(b)
    return tuple((pa[i] + pb[i]) / 2.0 for i in range(3))


# faces: (axis, side); corners in cyclic order around the face
FACES = []
for _d in range(3):
    _o1, _o2 = [a for a in range(3) if a != _d]
    for _s in range(2):
        cyc = []
        for (u, v) in ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = [0, 0, 0]
            p[_d], p[_o1], p[_o2] = _s, u, v
            cyc.append(_corner(p))
        FACES.append((_d, _s, cyc))


def _edge_between(c0, c1):
    for e in range(12):
        if set(edge_corners(e)) == {c0, c1}:
            return e
    raise AssertionError((c0, c1))


def _sub(a, b):
    return tuple(a[i] - b[i] for i in range(3))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(a[i] * b[i] for i in range(3))


def face_segments(case, face):
    """Directed segments (p, q) of one face of a case, by the face rule."""
    d, s, cyc = face
    inside = [(case >> c) & 1 for c in cyc]
    sides = [_edge_between(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]   # side i joins cyc[i] and cyc[i+1]
    crossed = [i for i in range(4) if inside[i] != inside[(i + 1) % 4]]
    n_face = [0, 0, 0]
    n_face[d] = 1 if s else -1                                            # outward normal of the face
    segs = []
    if len(crossed) == 2:
        ins = [corner_pos(cyc[i]) for i in range(4) if inside[i]]
        pairs = [((sides[crossed[0]], sides[crossed[1]]), ins)]
    elif len(crossed) == 4:
        # ambiguous: each inside corner i is cut off by the segment between its two sides (i-1 and i)
        pairs = [((sides[(i - 1) % 4], sides[i]), [corner_pos(cyc[i])]) for i in range(4) if inside[i]]
    else:
        pairs = []
    for (p, q), ins in pairs:
        P, Q = edge_mid(p), edge_mid(q)
        C = tuple(sum(c[i] for c in ins) / len(ins) for i in range(3))
        side = _dot(_cross(_sub(Q, P), tuple(n_face)), _sub(C, P))
        assert side != 0
        segs.append((p, q) if side > 0 else (q, p))
    return segs


def case_loops(case):
    segs = [sg for f in FACES for sg in face_segments(case, f)]
    nxt = {}
    for p, q in segs:
        assert p not in nxt, (case, p)
        nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def _faces_of(e):
    a, b = edge_corners(e)
    return {f for f, (_, _, cyc) in enumerate(FACES) if a in cyc and b in cyc}


def fan_start(loop):
    """The loop rotated to start at its first edge (see above)."""
    for e in sorted(loop):
        s = loop.index(e)
        rot = loop[s:] + loop[:s]
        if all(not (_faces_of(rot[0]) & _faces_of(rot[i])) for i in range(2, len(rot) - 1)):
            return rot
    raise AssertionError(loop)


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        loop = fan_start(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


TRIS = [case_triangles(c) for c in range(256)]
TRI_COUNT = [len(t) for t in TRIS]
MAX_TRIS = max(TRI_COUNT)

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudadepthmapintegration_amd", "csrc",
                   "isosurface_table.inc")


def render():
    lines = ["// GENERATED by tools/gen_mc_table.py -- do not edit.",
             "// Marching-cubes case table: corner c = x + 2y + 4z, case bit c set = corner inside (value >= iso).",
             "// clang-format off",
             "",
             "// edge e: axis, then the offset (x, y, z) of its lower corner within the cell",
             "constexpr int kMcEdges[12][4] = {"]
    for d, off in EDGES:
        lines.append("  {%d, %d, %d, %d}," % (d, off[0], off[1], off[2]))
    lines.append("};")
    lines.append("")
    lines.append("constexpr int kMcMaxTris = %d;  // most triangles of one case" % MAX_TRIS)
    lines.append("")
    lines.append("// triangles of each case")
    lines.append("constexpr unsigned char kMcTriCount[256] = {")
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join(str(n) for n in TRI_COUNT[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// edges of each triangle, in table order; unused entries are 0")
    lines.append("constexpr unsigned char kMcTriEdges[256][%d] = {" % (3 * MAX_TRIS))
    for c in range(256):
        flat = [e for t in TRIS[c] for e in t]
        flat += [0] * (3 * MAX_TRIS - len(flat))
        lines.append("  {" + ", ".join(str(e) for e in flat) + "},  // %d" % c)
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        fh.write(render())
    hist = [TRI_COUNT.count(n) for n in range(MAX_TRIS + 1)]
    print("wrote %s: at most %d triangles per cell; cases per triangle count %s" % (OUT, MAX_TRIS, hist))
