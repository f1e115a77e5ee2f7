"""Generator of the 256-case marching-cubes table compiled into moda_amd/csrc/mesh_kernels.hip.

Cell layout (shared by the kernels, tests/mc_numpy.py and this generator):
  corner c = (c & 1, (c >> 1) & 1, (c >> 2) & 1): its offset along array axes (0, 1, 2) from the cell's lower lattice point;
  edge e = 4 d + q runs along axis d from the corner whose offsets on the other two axes (a1 < a2) are (q & 1, q >> 1) and
  whose offset along d is 0.  bit c of a case index is set when corner c is occupied.

Per case, each of the cube's six faces contributes segments between the crossing points of its edges (an edge crosses
when its two corners differ in occupancy).  A face with two crossings gets one segment.  A face with four (two occupied
corners on a diagonal) is ambiguous; the fixed rule here is that occupied corners are NOT joined across the face: each
occupied corner is cut off by its own segment.  The rule reads only that face's four corners, so the two cells that
share a face always draw the same segments there and the mesh has no cracks.  Every crossing edge lies on two faces, so
the segments form closed loops.  Each segment is directed so that the loop's normal (right-hand rule) points from the
occupied side to the empty side.  Loops come in order of their lowest edge index; each is walked from that edge and
triangulated as a fan (l0, li, li+1) from its first point whose fan draws no diagonal between two points on one cube face
(such a diagonal could coincide with the neighbouring cell's and leave an edge shared by four triangles).  This differs
from PyMCubes' table in the ambiguous cases; it does not change which edges carry vertices.

`python -m moda_amd.mc_table` prints the text that sits between the marker comments in mesh_kernels.hip.
"""
import numpy as np

BEGIN = "// BEGIN GENERATED MC TABLE (python -m moda_amd.mc_table)"
END = "// END GENERATED MC TABLE"


def _corner(o):
    return o[0] | (o[1] << 1) | (o[2] << 2)


CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
EDGES = []          # (d, base offset (3,), corner0, corner1)
for _d in range(3):
    _a1, _a2 = [a for a in range(3) if a != _d]
    for _q in range(4):
        _o = [0, 0, 0]
        _o[_a1], _o[_a2] = _q & 1, _q >> 1
        _o1 = list(_o)
        _o1[_d] = 1
        EDGES.append((_d, tuple(_o), _corner(_o), _corner(_o1)))


def _mid(e):
    d, o, _, _ = EDGES[e]
    p = np.asarray(o, np.float64)
    p[d] += 0.5
    return p


def _segments(case):
    """Directed segments (from_edge, to_edge) of one case."""
    occ = [(case >> c) & 1 for c in range(8)]
    segs = []
    for a in range(3):
        for s in range(2):
            n = np.zeros(3)
            n[a] = 2 * s - 1                                           # outward normal of the face
            corners = [c for c in range(8) if CORNERS[c][a] == s]
            fedges = [e for e in range(12) if EDGES[e][0] != a and EDGES[e][1][a] == s]
            cross = [e for e in fedges if occ[EDGES[e][2]] != occ[EDGES[e][3]]]
            pos = {c: np.asarray(CORNERS[c], np.float64) for c in corners}
            pairs = []                                                 # (edge, edge, N: in-plane, occupied -> empty)
            if len(cross) == 2:
                full = [pos[c] for c in corners if occ[c]]
                empty = [pos[c] for c in corners if not occ[c]]
                pairs.append((cross[0], cross[1], np.mean(empty, 0) - np.mean(full, 0)))
            elif len(cross) == 4:
                centre = np.mean([pos[c] for c in corners], 0)
                for c in corners:
                    if occ[c]:
                        inc = [e for e in fedges if c in EDGES[e][2:]]
                        pairs.append((inc[0], inc[1], centre - pos[c]))
            else:
                assert not cross
            for e0, e1, N in pairs:
                T = np.cross(N, n)
                if np.dot(_mid(e1) - _mid(e0), T) < 0:
                    e0, e1 = e1, e0
                segs.append((e0, e1))
    return segs


def case_loops(case):
    """The closed loops of one case, each a list of edge indices starting at its lowest edge."""
    nxt = {}
    for e0, e1 in _segments(case):
        assert e0 not in nxt, (case, e0)
        nxt[e0] = e1
    assert sorted(nxt) == sorted(nxt.values()), case
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, case
        loops.append(loop)
    return loops


def _cube_faces(e):
    d, o, _, _ = EDGES[e]
    return {(a, o[a]) for a in range(3) if a != d}


def _fan_rotation(loop):
    """The loop rotated to its first point (in loop order from the lowest edge) whose fan draws no diagonal between two
    points on a common cube face: the cell across that face could draw the same segment, and the edge would then belong
    to four triangles.  Every loop of the 256 cases has such a point."""
    n = len(loop)
    for r in range(n):
        lr = loop[r:] + loop[:r]
        if all(not (_cube_faces(lr[0]) & _cube_faces(lr[i])) for i in range(2, n - 1)):
            return lr
    raise AssertionError(f"no face-safe fan for loop {loop}")


def generate():
    """(ntri (256,) int, tris (256, max_tri, 3) int with -1 padding): the triangles of each case as edge indices."""
    per_case = []
    for case in range(256):
        tri = []
        for loop in case_loops(case):
            loop = _fan_rotation(loop)
            tri += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
        per_case.append(tri)
    max_tri = max(len(t) for t in per_case)
    ntri = np.asarray([len(t) for t in per_case], np.int64)
    tris = -np.ones((256, max_tri, 3), np.int64)
    for case, t in enumerate(per_case):
        if t:
            tris[case, :len(t)] = t
    return ntri, tris


def table_text():
    """The C++ text between the markers in mesh_kernels.hip (markers included)."""
    ntri, tris = generate()
    max_tri = tris.shape[1]
    out = [BEGIN, f"constexpr int kMcMaxTri = {max_tri};",
           "// kMcEdge[e] = {axis, offset0, offset1, offset2} of the edge's lower corner",
           "__constant__ signed char kMcEdge[12][4] = {"]
    out.append("    " + ", ".join("{%d, %d, %d, %d}" % ((d,) + o) for d, o, _, _ in EDGES) + "};")
    out.append("__constant__ signed char kMcNumTri[256] = {")
    for r in range(0, 256, 32):
        out.append("    " + ", ".join(str(int(v)) for v in ntri[r:r + 32]) + ",")
    out.append("};")
    out.append("__constant__ signed char kMcTri[256][kMcMaxTri * 3] = {")
    for case in range(256):
        out.append("    {" + ", ".join(str(int(v)) for v in tris[case].reshape(-1)) + "},")
    out.append("};")
    out.append(END)
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    print(table_text(), end="")
