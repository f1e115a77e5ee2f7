// Mesh extraction after the lattice queries (reference nnutils/train_utils.py:1407-1451): the visibility mask fused into
// the reads (:1425), marching cubes (:1441) with the index-to-world affine (:1442), and the largest connected part
// (use_cc, :1447-1451).  Memory- and launch-bound: no MFMA.
//
//   classify   one thread per lattice point: the crossing mask of its +x/+y/+z edges (uint8, 3 bits), the case index of
//              the cell it is the lower corner of (uint8), and the occupied count (integer atomics, order-free)
//   scan       device-wide exclusive scans of popcount(mask) -> first vertex id per point and of kMcNumTri[case] -> first
//              face per cell: per-tile sums, one block scanning the tile sums, per-tile scans (no atomics: the output
//              is the same bit for bit on every run)
//   emit       one thread per point writes its vertices; one thread per cell writes its triangles.  The vertex id of edge
//              (point q, axis d) is voff[q] + popcount(mask[q] & ((1 << d) - 1)): mask + voff are the per-edge id array
//   largest    union-find over the vertices (two hooks per face, atomicMin on int32 parents, finds with plain loads
//              and no writes; a root always hooks under a smaller root, so every part ends with its lowest vertex as root whatever order the atomics ran
//              in), a vertex histogram per root, the (count, lowest index) maximum, then the same scans compact the
//              kept vertices and faces in their original order.
// Device memory is written only by plain stores and HIP atomic functions.  All indices are int32 (the entry points
// refuse 3 * g0 * g1 * g2 >= 2^31); byte offsets of the outputs are formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 8;
constexpr int kTile = kBlock * kPerThread;           // MODA_MC_SCAN_TILE

// BEGIN GENERATED MC TABLE (python -m moda_amd.mc_table)
constexpr int kMcMaxTri = 5;
// kMcEdge[e] = {axis, offset0, offset1, offset2} of the edge's lower corner
__constant__ signed char kMcEdge[12][4] = {
    {0, 0, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}, {0, 0, 1, 1}, {1, 0, 0, 0}, {1, 1, 0, 0}, {1, 0, 0, 1}, {1, 1, 0, 1}, {2, 0, 0, 0}, {2, 1, 0, 0}, {2, 0, 1, 0}, {2, 1, 1, 0}};
__constant__ signed char kMcNumTri[256] = {
    0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 2, 1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 2, 3, 4, 4, 3, 3, 4, 4, 3, 4, 5, 5, 2,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 2, 4, 3, 3, 4, 4, 5, 4, 3, 5, 2,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4, 3, 4, 4, 3, 4, 3, 5, 2, 4, 5, 5, 4, 5, 4, 2, 1,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 2, 3, 4, 5, 3, 2, 3, 4, 4, 3, 4, 5, 5, 4, 4, 5, 3, 2, 5, 2, 4, 1,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 2, 3, 3, 2, 3, 4, 4, 5, 4, 3, 5, 4, 4, 5, 5, 2, 3, 2, 4, 1,
    3, 4, 4, 5, 4, 5, 5, 2, 4, 5, 3, 4, 3, 4, 2, 1, 2, 3, 3, 2, 3, 2, 4, 1, 3, 4, 2, 1, 2, 1, 1, 0,
};
__constant__ signed char kMcTri[256][kMcMaxTri * 3] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 8, 1, 8, 9, 1, 9, 5, -1, -1, -1, -1, -1, -1},
    {1, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 11, 0, 11, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 9, 1, 9, 11, -1, -1, -1, -1, -1, -1},
    {4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 11, 0, 11, 10, 0, 10, 8, -1, -1, -1, -1, -1, -1},
    {0, 9, 11, 0, 11, 10, 0, 10, 4, -1, -1, -1, -1, -1, -1},
    {8, 9, 11, 8, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 9, 5, 2, 5, 4, 2, 4, 6, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 10, 4, 2, 8, 6, -1, -1, -1, -1, -1, -1},
    {1, 10, 6, 1, 6, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1},
    {1, 5, 11, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 2, 1, 5, 11, -1, -1, -1, -1, -1, -1},
    {0, 9, 11, 0, 11, 1, 2, 8, 6, -1, -1, -1, -1, -1, -1},
    {1, 4, 6, 1, 6, 2, 1, 2, 9, 1, 9, 11, -1, -1, -1},
    {2, 8, 6, 4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1},
    {0, 5, 11, 0, 11, 10, 0, 10, 6, 0, 6, 2, -1, -1, -1},
    {0, 9, 11, 0, 11, 10, 0, 10, 4, 2, 8, 6, -1, -1, -1},
    {2, 9, 11, 2, 11, 10, 2, 10, 6, -1, -1, -1, -1, -1, -1},
    {2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 2, 7, 0, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 7, 5, 2, 5, 4, 2, 4, 8, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 8, 2, 7, 9, -1, -1, -1, -1, -1, -1},
    {0, 2, 7, 0, 7, 5, 1, 10, 4, -1, -1, -1, -1, -1, -1},
    {1, 10, 8, 1, 8, 2, 1, 2, 7, 1, 7, 5, -1, -1, -1},
    {1, 5, 11, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 11, 2, 7, 9, -1, -1, -1, -1, -1, -1},
    {0, 2, 7, 0, 7, 11, 0, 11, 1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 2, 1, 2, 7, 1, 7, 11, -1, -1, -1},
    {2, 7, 9, 4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1},
    {0, 5, 11, 0, 11, 10, 0, 10, 8, 2, 7, 9, -1, -1, -1},
    {0, 2, 7, 0, 7, 11, 0, 11, 10, 0, 10, 4, -1, -1, -1},
    {2, 7, 11, 2, 11, 10, 2, 10, 8, -1, -1, -1, -1, -1, -1},
    {6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 7, 0, 7, 9, -1, -1, -1, -1, -1, -1},
    {0, 8, 6, 0, 6, 7, 0, 7, 5, -1, -1, -1, -1, -1, -1},
    {4, 6, 7, 4, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, 6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 9, -1, -1, -1},
    {0, 8, 6, 0, 6, 7, 0, 7, 5, 1, 10, 4, -1, -1, -1},
    {1, 10, 6, 1, 6, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1},
    {1, 5, 11, 6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 7, 0, 7, 9, 1, 5, 11, -1, -1, -1},
    {0, 8, 6, 0, 6, 7, 0, 7, 11, 0, 11, 1, -1, -1, -1},
    {1, 4, 6, 1, 6, 7, 1, 7, 11, -1, -1, -1, -1, -1, -1},
    {4, 5, 11, 4, 11, 10, 6, 7, 9, 6, 9, 8, -1, -1, -1},
    {0, 5, 11, 0, 11, 10, 0, 10, 6, 0, 6, 7, 0, 7, 9},
    {0, 8, 6, 0, 6, 7, 0, 7, 11, 0, 11, 10, 0, 10, 4},
    {6, 7, 11, 6, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 6, 10, 4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1},
    {1, 3, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 3, 0, 3, 6, 0, 6, 8, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 3, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1},
    {1, 3, 6, 1, 6, 8, 1, 8, 9, 1, 9, 5, -1, -1, -1},
    {1, 5, 11, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 11, 3, 6, 10, -1, -1, -1, -1, -1, -1},
    {0, 9, 11, 0, 11, 1, 3, 6, 10, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 9, 1, 9, 11, 3, 6, 10, -1, -1, -1},
    {3, 6, 4, 3, 4, 5, 3, 5, 11, -1, -1, -1, -1, -1, -1},
    {0, 5, 11, 0, 11, 3, 0, 3, 6, 0, 6, 8, -1, -1, -1},
    {0, 9, 11, 0, 11, 3, 0, 3, 6, 0, 6, 4, -1, -1, -1},
    {3, 6, 8, 3, 8, 9, 3, 9, 11, -1, -1, -1, -1, -1, -1},
    {2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 10, 0, 10, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1},
    {2, 9, 5, 2, 5, 4, 2, 4, 10, 2, 10, 3, -1, -1, -1},
    {1, 3, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1, -1, -1, -1},
    {0, 1, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 3, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1},
    {1, 3, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1, -1, -1, -1},
    {1, 5, 11, 2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1},
    {0, 4, 10, 0, 10, 3, 0, 3, 2, 1, 5, 11, -1, -1, -1},
    {0, 9, 11, 0, 11, 1, 2, 8, 10, 2, 10, 3, -1, -1, -1},
    {4, 10, 3, 4, 3, 2, 4, 2, 9, 4, 9, 11, 4, 11, 1},
    {2, 8, 4, 2, 4, 5, 2, 5, 11, 2, 11, 3, -1, -1, -1},
    {0, 5, 11, 0, 11, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1},
    {11, 3, 2, 11, 2, 8, 11, 8, 4, 11, 4, 0, 11, 0, 9},
    {2, 9, 11, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1},
    {0, 2, 7, 0, 7, 5, 3, 6, 10, -1, -1, -1, -1, -1, -1},
    {2, 7, 5, 2, 5, 4, 2, 4, 8, 3, 6, 10, -1, -1, -1},
    {1, 3, 6, 1, 6, 4, 2, 7, 9, -1, -1, -1, -1, -1, -1},
    {0, 1, 3, 0, 3, 6, 0, 6, 8, 2, 7, 9, -1, -1, -1},
    {0, 2, 7, 0, 7, 5, 1, 3, 6, 1, 6, 4, -1, -1, -1},
    {1, 3, 6, 1, 6, 8, 1, 8, 2, 1, 2, 7, 1, 7, 5},
    {1, 5, 11, 2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 11, 2, 7, 9, 3, 6, 10, -1, -1, -1},
    {0, 2, 7, 0, 7, 11, 0, 11, 1, 3, 6, 10, -1, -1, -1},
    {1, 4, 8, 1, 8, 2, 1, 2, 7, 1, 7, 11, 3, 6, 10},
    {2, 7, 9, 3, 6, 4, 3, 4, 5, 3, 5, 11, -1, -1, -1},
    {0, 5, 11, 0, 11, 3, 0, 3, 6, 0, 6, 8, 2, 7, 9},
    {0, 2, 7, 0, 7, 11, 0, 11, 3, 0, 3, 6, 0, 6, 4},
    {11, 3, 6, 11, 6, 8, 11, 8, 2, 11, 2, 7, -1, -1, -1},
    {3, 7, 9, 3, 9, 8, 3, 8, 10, -1, -1, -1, -1, -1, -1},
    {0, 4, 10, 0, 10, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1},
    {0, 8, 10, 0, 10, 3, 0, 3, 7, 0, 7, 5, -1, -1, -1},
    {3, 7, 5, 3, 5, 4, 3, 4, 10, -1, -1, -1, -1, -1, -1},
    {1, 3, 7, 1, 7, 9, 1, 9, 8, 1, 8, 4, -1, -1, -1},
    {0, 1, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1, -1, -1, -1},
    {8, 4, 1, 8, 1, 3, 8, 3, 7, 8, 7, 5, 8, 5, 0},
    {1, 3, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 11, 3, 7, 9, 3, 9, 8, 3, 8, 10, -1, -1, -1},
    {0, 4, 10, 0, 10, 3, 0, 3, 7, 0, 7, 9, 1, 5, 11},
    {0, 8, 10, 0, 10, 3, 0, 3, 7, 0, 7, 11, 0, 11, 1},
    {4, 10, 3, 4, 3, 7, 4, 7, 11, 4, 11, 1, -1, -1, -1},
    {3, 7, 9, 3, 9, 8, 3, 8, 4, 3, 4, 5, 3, 5, 11},
    {0, 5, 11, 0, 11, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1},
    {0, 8, 4, 3, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 11, 7, 4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 8, 3, 11, 7, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 10, 4, 3, 11, 7, -1, -1, -1, -1, -1, -1},
    {1, 10, 8, 1, 8, 9, 1, 9, 5, 3, 11, 7, -1, -1, -1},
    {1, 5, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1},
    {0, 9, 7, 0, 7, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 9, 1, 9, 7, 1, 7, 3, -1, -1, -1},
    {3, 10, 4, 3, 4, 5, 3, 5, 7, -1, -1, -1, -1, -1, -1},
    {0, 5, 7, 0, 7, 3, 0, 3, 10, 0, 10, 8, -1, -1, -1},
    {0, 9, 7, 0, 7, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1},
    {3, 10, 8, 3, 8, 9, 3, 9, 7, -1, -1, -1, -1, -1, -1},
    {2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 2, 3, 11, 7, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1},
    {2, 9, 5, 2, 5, 4, 2, 4, 6, 3, 11, 7, -1, -1, -1},
    {1, 10, 4, 2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 6, 0, 6, 2, 3, 11, 7, -1, -1, -1},
    {0, 9, 5, 1, 10, 4, 2, 8, 6, 3, 11, 7, -1, -1, -1},
    {1, 10, 6, 1, 6, 2, 1, 2, 9, 1, 9, 5, 3, 11, 7},
    {1, 5, 7, 1, 7, 3, 2, 8, 6, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 2, 1, 5, 7, 1, 7, 3, -1, -1, -1},
    {0, 9, 7, 0, 7, 3, 0, 3, 1, 2, 8, 6, -1, -1, -1},
    {1, 4, 6, 1, 6, 2, 1, 2, 9, 1, 9, 7, 1, 7, 3},
    {2, 8, 6, 3, 10, 4, 3, 4, 5, 3, 5, 7, -1, -1, -1},
    {0, 5, 7, 0, 7, 3, 0, 3, 10, 0, 10, 6, 0, 6, 2},
    {0, 9, 7, 0, 7, 3, 0, 3, 10, 0, 10, 4, 2, 8, 6},
    {9, 7, 3, 9, 3, 10, 9, 10, 6, 9, 6, 2, -1, -1, -1},
    {2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1},
    {0, 2, 3, 0, 3, 11, 0, 11, 5, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, 2, 11, 5, 2, 5, 4, 2, 4, 8, -1, -1, -1},
    {1, 10, 4, 2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 8, 2, 3, 11, 2, 11, 9, -1, -1, -1},
    {0, 2, 3, 0, 3, 11, 0, 11, 5, 1, 10, 4, -1, -1, -1},
    {8, 2, 3, 8, 3, 11, 8, 11, 5, 8, 5, 1, 8, 1, 10},
    {1, 5, 9, 1, 9, 2, 1, 2, 3, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 9, 1, 9, 2, 1, 2, 3, -1, -1, -1},
    {0, 2, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 2, 1, 2, 3, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 2, 10, 4, 2, 4, 5, 2, 5, 9, -1, -1, -1},
    {5, 9, 2, 5, 2, 3, 5, 3, 10, 5, 10, 8, 5, 8, 0},
    {0, 2, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1, -1, -1, -1},
    {2, 3, 10, 2, 10, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 11, 9, 3, 9, 8, 3, 8, 6, -1, -1, -1, -1, -1, -1},
    {0, 4, 6, 0, 6, 3, 0, 3, 11, 0, 11, 9, -1, -1, -1},
    {0, 8, 6, 0, 6, 3, 0, 3, 11, 0, 11, 5, -1, -1, -1},
    {3, 11, 5, 3, 5, 4, 3, 4, 6, -1, -1, -1, -1, -1, -1},
    {1, 10, 4, 3, 11, 9, 3, 9, 8, 3, 8, 6, -1, -1, -1},
    {0, 1, 10, 0, 10, 6, 0, 6, 3, 0, 3, 11, 0, 11, 9},
    {0, 8, 6, 0, 6, 3, 0, 3, 11, 0, 11, 5, 1, 10, 4},
    {6, 3, 11, 6, 11, 5, 6, 5, 1, 6, 1, 10, -1, -1, -1},
    {1, 5, 9, 1, 9, 8, 1, 8, 6, 1, 6, 3, -1, -1, -1},
    {6, 3, 1, 6, 1, 5, 6, 5, 9, 6, 9, 0, 6, 0, 4},
    {0, 8, 6, 0, 6, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1},
    {1, 4, 6, 1, 6, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 10, 4, 3, 4, 5, 3, 5, 9, 3, 9, 8, 3, 8, 6},
    {0, 5, 9, 3, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 6, 0, 6, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1},
    {3, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1},
    {4, 8, 9, 4, 9, 5, 6, 10, 11, 6, 11, 7, -1, -1, -1},
    {1, 11, 7, 1, 7, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1},
    {0, 1, 11, 0, 11, 7, 0, 7, 6, 0, 6, 8, -1, -1, -1},
    {0, 9, 5, 1, 11, 7, 1, 7, 6, 1, 6, 4, -1, -1, -1},
    {1, 11, 7, 1, 7, 6, 1, 6, 8, 1, 8, 9, 1, 9, 5},
    {1, 5, 7, 1, 7, 6, 1, 6, 10, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 1, 5, 7, 1, 7, 6, 1, 6, 10, -1, -1, -1},
    {0, 9, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1},
    {1, 4, 8, 1, 8, 9, 1, 9, 7, 1, 7, 6, 1, 6, 10},
    {4, 5, 7, 4, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 7, 0, 7, 6, 0, 6, 8, -1, -1, -1, -1, -1, -1},
    {0, 9, 7, 0, 7, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1},
    {6, 8, 9, 6, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 10, 2, 10, 11, 2, 11, 7, -1, -1, -1, -1, -1, -1},
    {0, 4, 10, 0, 10, 11, 0, 11, 7, 0, 7, 2, -1, -1, -1},
    {0, 9, 5, 2, 8, 10, 2, 10, 11, 2, 11, 7, -1, -1, -1},
    {2, 9, 5, 2, 5, 4, 2, 4, 10, 2, 10, 11, 2, 11, 7},
    {1, 11, 7, 1, 7, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1},
    {0, 1, 11, 0, 11, 7, 0, 7, 2, -1, -1, -1, -1, -1, -1},
    {0, 9, 5, 1, 11, 7, 1, 7, 2, 1, 2, 8, 1, 8, 4},
    {1, 11, 7, 1, 7, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1},
    {1, 5, 7, 1, 7, 2, 1, 2, 8, 1, 8, 10, -1, -1, -1},
    {10, 1, 5, 10, 5, 7, 10, 7, 2, 10, 2, 0, 10, 0, 4},
    {7, 2, 8, 7, 8, 10, 7, 10, 1, 7, 1, 0, 7, 0, 9},
    {1, 4, 10, 2, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 4, 2, 4, 5, 2, 5, 7, -1, -1, -1, -1, -1, -1},
    {0, 5, 7, 0, 7, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {7, 2, 8, 7, 8, 4, 7, 4, 0, 7, 0, 9, -1, -1, -1},
    {2, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 6, 10, 2, 10, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1},
    {0, 4, 8, 2, 6, 10, 2, 10, 11, 2, 11, 9, -1, -1, -1},
    {0, 2, 6, 0, 6, 10, 0, 10, 11, 0, 11, 5, -1, -1, -1},
    {2, 6, 10, 2, 10, 11, 2, 11, 5, 2, 5, 4, 2, 4, 8},
    {1, 11, 9, 1, 9, 2, 1, 2, 6, 1, 6, 4, -1, -1, -1},
    {1, 11, 9, 1, 9, 2, 1, 2, 6, 1, 6, 8, 1, 8, 0},
    {2, 6, 4, 2, 4, 1, 2, 1, 11, 2, 11, 5, 2, 5, 0},
    {1, 11, 5, 2, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 9, 1, 9, 2, 1, 2, 6, 1, 6, 10, -1, -1, -1},
    {0, 4, 8, 1, 5, 9, 1, 9, 2, 1, 2, 6, 1, 6, 10},
    {0, 2, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 1, 8, 2, 1, 2, 6, 1, 6, 10, -1, -1, -1},
    {2, 6, 4, 2, 4, 5, 2, 5, 9, -1, -1, -1, -1, -1, -1},
    {5, 9, 2, 5, 2, 6, 5, 6, 8, 5, 8, 0, -1, -1, -1},
    {0, 2, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 10, 11, 8, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 4, 10, 0, 10, 11, 0, 11, 9, -1, -1, -1, -1, -1, -1},
    {0, 8, 10, 0, 10, 11, 0, 11, 5, -1, -1, -1, -1, -1, -1},
    {4, 10, 11, 4, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 9, 1, 9, 8, 1, 8, 4, -1, -1, -1, -1, -1, -1},
    {0, 1, 11, 0, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 4, 1, 8, 1, 11, 8, 11, 5, 8, 5, 0, -1, -1, -1},
    {1, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 9, 1, 9, 8, 1, 8, 10, -1, -1, -1, -1, -1, -1},
    {10, 1, 5, 10, 5, 9, 10, 9, 0, 10, 0, 4, -1, -1, -1},
    {0, 8, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 9, 4, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};
// END GENERATED MC TABLE

DEVINL float mc_value(const float* __restrict__ vol, const float* __restrict__ vis, long long p) {
    const float v = vol[p];
    return (vis != nullptr && vis[p] < 0.5f) ? -1.f : v;             // :1425, fused into the read
}

DEVINL bool mc_occupied(float v, float thr) { return isfinite(v) && v > thr; }   // :1435 (strict >); not finite: empty

// ---- classify ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mc_classify_kernel(const float* __restrict__ vol, const float* __restrict__ vis,
                                                             int g0, int g1, int g2, float thr, uint8_t* __restrict__ mask,
                                                             uint8_t* __restrict__ ccase,
                                                             unsigned long long* __restrict__ n_occ) {
    const int n = g0 * g1 * g2;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    int occ_here = 0;
    if (p < n) {
        const int k = p % g2, j = (p / g2) % g1, i = p / (g1 * g2);
        const int s1 = g2, s0 = g1 * g2;
        const bool hx = i + 1 < g0, hy = j + 1 < g1, hz = k + 1 < g2;
        int occ[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
            const bool in = (!dx || hx) && (!dy || hy) && (!dz || hz);
            occ[c] = in ? (int)mc_occupied(mc_value(vol, vis, (long long)p + dx * s0 + dy * s1 + dz), thr) : occ[0];
        }
        occ_here = occ[0];
        mask[p] = (uint8_t)((hx && occ[1] != occ[0] ? 1 : 0) | (hy && occ[2] != occ[0] ? 2 : 0) | (hz && occ[4] != occ[0] ? 4 : 0));
        if (hx && hy && hz) {
            int cs = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) cs |= occ[c] << c;
            ccase[(i * (g1 - 1) + j) * (g2 - 1) + k] = (uint8_t)cs;
        }
    }
    const int cnt = __syncthreads_count(occ_here);
    if (threadIdx.x == 0 && cnt) atomicAdd(n_occ, (unsigned long long)cnt);
}

// ---- device-wide exclusive scan of int counts (tile = 2048 items) ------------------------------------------------
struct CountBits {           // vertices per lattice point
    const uint8_t* m;
    DEVINL int operator()(int i) const { return __popc((unsigned)m[i]); }
};
struct CountTris {           // triangles per cell
    const uint8_t* c;
    DEVINL int operator()(int i) const { return kMcNumTri[c[i]]; }
};
DEVINL int best_root(const unsigned long long* key) { return 0x7fffffff - (int)(unsigned)(*key & 0xffffffffull); }
struct KeepVertex {          // vertex in the chosen part
    const int* label; const unsigned long long* key;
    DEVINL int operator()(int i) const { return label[i] == best_root(key) ? 1 : 0; }
};
// a face whose three indices lie in [0, nv): the others are counted (totals[3]) and refused by the caller, never read through
DEVINL bool face_ok(const int* faces, long long f, int nv) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    return a >= 0 && b >= 0 && c >= 0 && a < nv && b < nv && c < nv;
}
struct KeepFace {            // face in the chosen part (its three vertices share one label)
    const int* label; const int* faces; const unsigned long long* key; int nv;
    DEVINL int operator()(int i) const { return face_ok(faces, i, nv) && label[faces[3LL * i]] == best_root(key) ? 1 : 0; }
};

// (the scans below are lanes.h's block_scan: the inclusive value of a thread is incl_wave + before)
template <class F>
__global__ __launch_bounds__(kBlock) void scan_tile_sum_kernel(F f, int n, int* __restrict__ tile_sum) {
    __shared__ int lds[kBlock / 64];
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int s = 0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q)
        if (base + q < n) s += f(base + q);
    const BlockScan<int> r = block_scan<int, kBlock / 64>(s, lds);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = r.total;
}

// one block: exclusive scan of the tile sums in 64 bits, total -> *total
__global__ __launch_bounds__(1024) void scan_tiles_kernel(const int* __restrict__ tile_sum, int nt, int64_t* __restrict__ tile_off,
                                                          int64_t* __restrict__ total) {
    __shared__ long long lds[1024 / 64];
    long long carry = 0;
    for (int b0 = 0; b0 < nt; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const long long own = b < nt ? (long long)tile_sum[b] : 0;
        const BlockScan<long long> r = block_scan<long long, 1024 / 64>(own, lds);
        if (b < nt) tile_off[b] = carry + r.before + r.incl_wave - own;
        carry += r.total;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class F>
__global__ __launch_bounds__(kBlock) void scan_tile_kernel(F f, int n, const int64_t* __restrict__ tile_off, int* __restrict__ out) {
    __shared__ int lds[kBlock / 64];
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int c[kPerThread];
    int s = 0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        c[q] = base + q < n ? f(base + q) : 0;
        s += c[q];
    }
    const BlockScan<int> r = block_scan<int, kBlock / 64>(s, lds);
    const int incl = r.incl_wave + r.before;
    long long run = tile_off[blockIdx.x] + (incl - s);
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        if (base + q < n) out[base + q] = (int)run;          // the entry points refuse totals >= 2^31 before anything reads these
        run += c[q];
    }
}

template <class F>
void exclusive_scan(F f, int n, int* tile_sum, int64_t* tile_off, int* out, int64_t* total, hipStream_t st) {
    const unsigned nt = nblocks(n, kTile);
    hipLaunchKernelGGL(scan_tile_sum_kernel<F>, dim3(nt), dim3(kBlock), 0, st, f, n, tile_sum);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, st, tile_sum, (int)nt, tile_off, total);
    hipLaunchKernelGGL(scan_tile_kernel<F>, dim3(nt), dim3(kBlock), 0, st, f, n, tile_off, out);
}

// ---- emit -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mc_vertex_kernel(const float* __restrict__ vol, const float* __restrict__ vis, int g0,
                                                           int g1, int g2, float thr, const uint8_t* __restrict__ mask,
                                                           const int* __restrict__ voff, double sx, double sy, double sz,
                                                           double tx, double ty, double tz, int nv, float* __restrict__ verts) {
    const int n = g0 * g1 * g2;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const unsigned m = mask[p];
    if (!m) return;
    const int k = p % g2, j = (p / g2) % g1, i = p / (g1 * g2);
    const int stride[3] = {g1 * g2, g2, 1};
    const float a = mc_value(vol, vis, p);
    int id = voff[p];
    const double sc[3] = {sx, sy, sz}, sh[3] = {tx, ty, tz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (!(m & (1u << d))) continue;
        const float b = mc_value(vol, vis, (long long)p + stride[d]);
        // t in double: exact differences of fp32 values, so no overflow for |v| near FLT_MAX, and one rounding
        double t;
        if (!isfinite(a)) t = 1.0;                                   // the finite end (b: a crossing has one occupied end)
        else if (!isfinite(b)) t = 0.0;
        else t = fmin(fmax(((double)thr - (double)a) / ((double)b - (double)a), 0.0), 1.0);
        if (id < nv) {
            float* o = verts + 3LL * id;
            const int ijk[3] = {i, j, k};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double pc = (double)ijk[c] + (c == d ? t : 0.0);
                o[c] = (float)(pc * sc[c] + sh[c]);                                   // one rounding to fp32 (:1442)
            }
        }
        ++id;
    }
}

__global__ __launch_bounds__(kBlock) void mc_face_kernel(int g0, int g1, int g2, const uint8_t* __restrict__ mask,
                                                         const int* __restrict__ voff, const uint8_t* __restrict__ ccase,
                                                         const int* __restrict__ foff, int nf, int* __restrict__ faces) {
    const int nc = (g0 - 1) * (g1 - 1) * (g2 - 1);
    const int cell = blockIdx.x * kBlock + threadIdx.x;
    if (cell >= nc) return;
    const int cs = ccase[cell];
    const int nt = kMcNumTri[cs];
    if (!nt) return;
    const int k = cell % (g2 - 1), j = (cell / (g2 - 1)) % (g1 - 1), i = cell / ((g1 - 1) * (g2 - 1));
    const int p = (i * g1 + j) * g2 + k;
    const int f0 = foff[cell];
    for (int s = 0; s < nt; ++s) {
        if (f0 + s >= nf) return;
        int* o = faces + 3LL * (f0 + s);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const int e = kMcTri[cs][3 * s + v];
            const int d = kMcEdge[e][0];
            const int q = p + kMcEdge[e][1] * g1 * g2 + kMcEdge[e][2] * g2 + kMcEdge[e][3];
            o[v] = voff[q] + __popc((unsigned)mask[q] & ((1u << d) - 1u));
        }
    }
}

// ---- largest connected part -------------------------------------------------------------------------------------
// Finds use plain loads and write nothing.  Within the hook launch a load may return an older parent (another CU's
// atomicMin not yet visible in this CU's L1).  That is harmless: a parent only ever decreases and always lies in the same
// part, so an older value is still a vertex of the part, and every hook that acts goes through atomicMin, whose return
// value is current.  A failed hook replaces the larger of its pair by a strictly smaller vertex, so the loop ends.
DEVINL int uf_find(const int* parent, int x) {
    int p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

__global__ __launch_bounds__(kBlock) void uf_init_kernel(int nv, int* __restrict__ parent, int* __restrict__ cnt,
                                                         unsigned long long* __restrict__ key) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) { parent[v] = v; cnt[v] = 0; }
    if (v == 0) { key[0] = 0ull; key[1] = 0ull; }                  // totals[2] (best key), totals[3] (bad faces)
}

DEVINL void uf_hook(int* parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);                  // hook the larger root under the smaller
        if (old == a) return;
        a = old;                                                   // a was hooked meanwhile: join its current parent and b
    }
}

// one thread per face: hooks (f0, f1) and (f1, f2); a face with an index outside [0, nv) is counted and skipped
__global__ __launch_bounds__(kBlock) void uf_hook_kernel(const int* __restrict__ faces, int nf, int nv, int* parent,
                                                         unsigned long long* __restrict__ n_bad) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    if (!face_ok(faces, f, nv)) {
        atomicAdd(n_bad, 1ull);
        return;
    }
    const int a = faces[3LL * f], b = faces[3LL * f + 1], c = faces[3LL * f + 2];
    uf_hook(parent, a, b);
    uf_hook(parent, b, c);
}

// label = root; histogram per root.  One part can hold nearly every vertex, so the adds are aggregated before they reach
// the one hot counter: runs of equal roots per thread (4 consecutive vertices), then per wave and root
constexpr int kLabelPer = 4;
__global__ __launch_bounds__(kBlock) void uf_label_kernel(int nv, const int* __restrict__ parent, int* __restrict__ label, int* __restrict__ cnt) {
    const int base = (blockIdx.x * kBlock + threadIdx.x) * kLabelPer;
    int cur = -1, run = 0;
    for (int q = 0; q < kLabelPer && base + q < nv; ++q) {
        const int r = uf_find(parent, base + q);                   // a new launch: every load is current
        label[base + q] = r;
        if (r != cur) {
            if (run) atomicAdd(cnt + cur, run);
            cur = r;
            run = 0;
        }
        ++run;
    }
    unsigned long long pending = __ballot(run > 0);
    while (pending) {                                              // wave-uniform: one iteration per distinct root
        const int rl = __shfl(cur, __builtin_ctzll(pending));
        const bool mine = run > 0 && cur == rl;
        const int tot = wave_add(mine ? run : 0);
        const unsigned long long same = __ballot(mine);
        if ((threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(cnt + rl, tot);
        pending &= ~same;
    }
}

__global__ __launch_bounds__(kBlock) void uf_best_kernel(int nv, const int* __restrict__ label, const int* __restrict__ cnt,
                                                         unsigned long long* __restrict__ key) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv || label[v] != v) return;
    // most vertices first, then the lowest root (= the part's lowest vertex index)
    atomicMax(key, ((unsigned long long)(unsigned)cnt[v] << 32) | (unsigned long long)(unsigned)(0x7fffffff - v));
}

__global__ __launch_bounds__(kBlock) void compact_vertex_kernel(int nv, const float* __restrict__ verts, const int* __restrict__ label,
                                                                const unsigned long long* __restrict__ key, const int* __restrict__ vnew,
                                                                float* __restrict__ out) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv || label[v] != best_root(key)) return;
    const long long o = 3LL * vnew[v];
    out[o] = verts[3LL * v]; out[o + 1] = verts[3LL * v + 1]; out[o + 2] = verts[3LL * v + 2];
}

__global__ __launch_bounds__(kBlock) void compact_face_kernel(int nf, int nv, const int* __restrict__ faces, const int* __restrict__ label,
                                                              const unsigned long long* __restrict__ key, const int* __restrict__ vnew,
                                                              const int* __restrict__ fnew, int* __restrict__ out) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf || !face_ok(faces, f, nv) || label[faces[3LL * f]] != best_root(key)) return;
    const long long o = 3LL * fnew[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o + c] = vnew[faces[3LL * f + c]];
}

bool mc_shape_ok(int64_t g0, int64_t g1, int64_t g2) {
    if (g0 < 2 || g1 < 2 || g2 < 2) return false;
    const double n3 = 3.0 * (double)g0 * (double)g1 * (double)g2;   // no int64 overflow for any int64 extents
    return n3 < 2147483648.0;
}

}   // namespace

extern "C" int moda_mc_count(const float* vol, const float* vis, int64_t g0, int64_t g1, int64_t g2, float threshold,
                             uint8_t* mask, uint8_t* cell_case, int32_t* voff, int32_t* foff, int32_t* tile_sum,
                             int64_t* tile_off, int64_t* totals, void* stream) {
    if (!mc_shape_ok(g0, g1, g2)) return MODA_ESHAPE;
    if (!vol || !mask || !cell_case || !voff || !foff || !tile_sum || !tile_off || !totals) return MODA_EINVAL;
    if (moda_stream_capture_id(stream) != 0) return MODA_EINVAL;    // the caller reads totals back: no graph capture
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)(g0 * g1 * g2), nc = (int)((g0 - 1) * (g1 - 1) * (g2 - 1));
    hipError_t e = hipMemsetAsync(totals + 2, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mc_classify_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, st, vol, vis, (int)g0, (int)g1, (int)g2,
                       threshold, mask, cell_case, (unsigned long long*)(totals + 2));
    exclusive_scan(CountBits{mask}, n, tile_sum, tile_off, voff, totals, st);
    exclusive_scan(CountTris{cell_case}, nc, tile_sum, tile_off, foff, totals + 1, st);
    return (int)hipGetLastError();
}

extern "C" int moda_mc_emit(const float* vol, const float* vis, int64_t g0, int64_t g1, int64_t g2, float threshold,
                            const uint8_t* mask, const uint8_t* cell_case, const int32_t* voff, const int32_t* foff,
                            double scale_x, double scale_y, double scale_z, double shift_x, double shift_y, double shift_z,
                            int64_t n_vertices, int64_t n_faces, float* vertices, int32_t* faces, void* stream) {
    if (!mc_shape_ok(g0, g1, g2)) return MODA_ESHAPE;
    if (n_vertices < 0 || n_faces < 0 || n_vertices >= 2147483648LL || n_faces >= 2147483648LL) return MODA_ESHAPE;
    if (!vol || !mask || !cell_case || !voff || !foff || (n_vertices && !vertices) || (n_faces && !faces)) return MODA_EINVAL;
    if (moda_stream_capture_id(stream) != 0) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)(g0 * g1 * g2), nc = (int)((g0 - 1) * (g1 - 1) * (g2 - 1));
    if (n_vertices)
        hipLaunchKernelGGL(mc_vertex_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, st, vol, vis, (int)g0, (int)g1, (int)g2,
                           threshold, mask, voff, scale_x, scale_y, scale_z, shift_x, shift_y, shift_z, (int)n_vertices, vertices);
    if (n_faces)
        hipLaunchKernelGGL(mc_face_kernel, dim3(nblocks(nc, kBlock)), dim3(kBlock), 0, st, (int)g0, (int)g1, (int)g2, mask, voff,
                           cell_case, foff, (int)n_faces, faces);
    return (int)hipGetLastError();
}

extern "C" int moda_mesh_largest_part(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                                      int32_t* parent, int32_t* label, int32_t* count, int32_t* vnew, int32_t* fnew,
                                      int32_t* tile_sum, int64_t* tile_off, int64_t* totals, float* vertices_out,
                                      int32_t* faces_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || n_vertices >= 2147483647LL || 2 * n_faces >= 2147483647LL) return MODA_ESHAPE;
    if (n_vertices == 0) return 0;
    if (!vertices || (n_faces && !faces) || !parent || !label || !count || !vnew || (n_faces && !fnew) || !tile_sum || !tile_off
        || !totals || !vertices_out || (n_faces && !faces_out))
        return MODA_EINVAL;
    if (moda_stream_capture_id(stream) != 0) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nv = (int)n_vertices, nf = (int)n_faces;
    unsigned long long* key = (unsigned long long*)(totals + 2);
    hipLaunchKernelGGL(uf_init_kernel, dim3(nblocks(nv, kBlock)), dim3(kBlock), 0, st, nv, parent, count, key);
    if (nf) {
        hipLaunchKernelGGL(uf_hook_kernel, dim3(nblocks(nf, kBlock)), dim3(kBlock), 0, st, faces, nf, nv, parent,
                           (unsigned long long*)(totals + 3));
    }
    hipLaunchKernelGGL(uf_label_kernel, dim3(nblocks(nv, kBlock * kLabelPer)), dim3(kBlock), 0, st, nv, parent, label, count);
    hipLaunchKernelGGL(uf_best_kernel, dim3(nblocks(nv, kBlock)), dim3(kBlock), 0, st, nv, label, count, key);
    exclusive_scan(KeepVertex{label, key}, nv, tile_sum, tile_off, vnew, totals, st);
    hipLaunchKernelGGL(compact_vertex_kernel, dim3(nblocks(nv, kBlock)), dim3(kBlock), 0, st, nv, vertices, label, key, vnew,
                       vertices_out);
    if (nf) {
        exclusive_scan(KeepFace{label, faces, key, nv}, nf, tile_sum, tile_off, fnew, totals + 1, st);
        hipLaunchKernelGGL(compact_face_kernel, dim3(nblocks(nf, kBlock)), dim3(kBlock), 0, st, nf, nv, faces, label, key, vnew, fnew,
                           faces_out);
    } else {
        hipError_t e = hipMemsetAsync(totals + 1, 0, sizeof(int64_t), st);
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipGetLastError();
}
