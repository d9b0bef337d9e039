"""Generate csrc/mc_tables.h: the marching-cubes case tables, derived by rule (none of them is typed in).

Cube conventions (shared with csrc/marching_cubes.hip and tests/mesh_model.py):
  corner c = bx | by << 1 | bz << 2, at offset (bx, by, bz) from the cell's origin;
  edge e = 4 a + o along axis a (x, y, z = 0, 1, 2); o = (offset on the first other axis) | (offset on the second) << 1,
           the other axes in increasing order; its lower endpoint is the corner with bit a clear;
  face f = 2 a + s: the face where corner bit a == s, outward normal (2 s - 1) e_a.
Case bit c is set iff corner c is inside (sigma > level).

The rule, per case:
  1. On every face, walk the four corners counter-clockwise as seen from outside the cube.  A crossing edge entered from an
     outside corner into an inside one is an ENTRY, the others EXITs.  Each entry is joined to the next exit along the walk:
     a segment entry -> exit that cuts off the run of inside corners between them.  On an ambiguous face (two diagonal
     inside corners) this separates the inside corners.  The segments of a face depend on that face's four corners only,
     so two cells that share a face put the same segments on it, traversed in opposite directions.
  2. A crossing edge lies on exactly two faces and is traversed in opposite directions by them: it is the exit of one
     segment and the entry of another, so the segments chain into disjoint loops.
  3. Loops are taken in order of their smallest edge and followed from it; each loop (l0, l1, ..., l(n-1)) is fanned into
     triangles (l0, li, l(i+1)).  With segments running entry -> exit the triangles face away from the inside corners:
     outward, towards lower sigma.

usage: python tools/make_mc_tables.py [--check]   (writes, or compares against, nerf-simple_amd/csrc/mc_tables.h)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "nerf-simple_amd", "csrc", "mc_tables.h")


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def other_axes(a):
    return [b for b in range(3) if b != a]


def edge_corners(e):
    """(lower corner, upper corner) of edge e"""
    a, o = divmod(e, 4)
    b, c = other_axes(a)
    lo = ((o & 1) << b) | (((o >> 1) & 1) << c)
    return lo, lo | (1 << a)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def face_walk(f):
    """corners of face f in counter-clockwise order seen from outside (right-hand rule about the outward normal)"""
    a, s = divmod(f, 2)
    b, c = (a + 1) % 3, (a + 2) % 3           # e_a x e_b = e_c: counter-clockwise about +e_a runs from e_b to e_c
    cyc = [(0, 0), (1, 0), (1, 1), (0, 1)]
    if s == 0:
        cyc = [cyc[0], cyc[3], cyc[2], cyc[1]]   # about -e_a the other way round
    return [(s << a) | (u << b) | (v << c) for u, v in cyc]


def face_edges(f):
    w = face_walk(f)
    return [EDGE_OF[frozenset((w[k], w[(k + 1) % 4]))] for k in range(4)]


def face_segments(f, inside):
    """directed segments (entry edge, exit edge) on face f; inside: 8 booleans"""
    w = face_walk(f)
    edges = face_edges(f)
    kind = []                                  # per walk step k (edge w[k] -> w[k+1]): 'in', 'out' or None
    for k in range(4):
        a, b = inside[w[k]], inside[w[(k + 1) % 4]]
        kind.append(None if a == b else ("in" if b else "out"))
    segs = []
    for k in range(4):
        if kind[k] == "in":
            j = (k + 1) % 4
            while kind[j] != "out":
                j = (j + 1) % 4
            segs.append((edges[k], edges[j]))
    return segs


def case_inside(case):
    return [bool((case >> c) & 1) for c in range(8)]


def crossing_edges(case):
    ins = case_inside(case)
    return [e for e in range(12) if ins[edge_corners(e)[0]] != ins[edge_corners(e)[1]]]


def case_segments(case):
    ins = case_inside(case)
    return {f: face_segments(f, ins) for f in range(6)}


def case_loops(case):
    nxt = {}
    for segs in case_segments(case).values():
        for a, b in segs:
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == crossing_edges(case) and sorted(nxt.values()) == crossing_edges(case), case
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop, x = [], e
        while x not in seen:
            seen.add(x)
            loop.append(x)
            x = nxt[x]
        assert x == e
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_tables():
    """-> (tri_count[256], triangles[256] as lists of (e0, e1, e2))"""
    tris = [case_triangles(c) for c in range(256)]
    return [len(t) for t in tris], tris


def render():
    counts, tris = build_tables()
    mx = max(counts)
    lines = [
        "// mc_tables.h -- GENERATED by tools/make_mc_tables.py; do not edit (tests/test_mesh_cpu.py checks it is current).",
        "// Marching-cubes tables derived by rule (the rule and the cube conventions: tools/make_mc_tables.py).",
        "//   corner c = bx | by << 1 | bz << 2;  edge e = 4 * axis + o (o: offsets on the two other axes, lower axis first);",
        "//   case bit c set iff corner c is inside (sigma > level).  Triangles face outward (towards lower sigma).",
        "#pragma once",
        "",
        "namespace mc_tables {",
        "",
        f"constexpr int MAX_TRIS = {mx};",
        "",
        "// lower corner of edge e (its upper corner is lower | 1 << (e / 4))",
        "__constant__ const unsigned char edge_lower[12] = {" + ", ".join(str(edge_corners(e)[0]) for e in range(12)) + "};",
        "",
        "// triangles per case",
        "__constant__ const unsigned char tri_count[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(x) for x in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"// edges of each case's triangles, 3 per triangle, in emission order; 255 pads to MAX_TRIS")
    lines.append(f"__constant__ const unsigned char tri_edges[256][{3 * mx}] = {{")
    for c in range(256):
        flat = [e for t in tris[c] for e in t]
        flat += [255] * (3 * mx - len(flat))
        lines.append("    {" + ", ".join(str(x) for x in flat) + "},")
    lines.append("};")
    lines.append("")
    lines.append("}  // namespace mc_tables")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv[1:]:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h is current" if same else "mc_tables.h differs from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(f"wrote {HEADER}")
