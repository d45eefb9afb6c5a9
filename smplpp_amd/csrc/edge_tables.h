// The edge table of a mesh and the launch plan of the geodesic relaxation (geodesic.hip): what
// smplpp_mesh_geodesic and smplpp_self_contact_create compute on the host before any kernel runs.  Plain C++17, no HIP: a CPU test
// runs the builder and the plan as a stand-alone program (tests/cpp/edge_tables_dump.cpp).
//
// THE RULE of smplpp_mesh_geodesic (include/smplpp_hip.h states it for callers):
//  edge length  w(u, v) = sqrtf((dx dx + dy dy) + dz dz), d = x_hi - x_lo, lo = min(u, v), hi = max(u, v): every operation rounded
//               on its own, the square root the correctly rounded one, so both directions of an edge carry the same bits.  A length
//               that is not finite (a NaN or inf coordinate, an overflow) is stored as +inf: the edge does not exist.  0 is a length.
//  distance     dist[v] = the minimum over all edge paths from a source of the set to v of the left-to-right fp32 sum of the path's
//               lengths, from +0 at the source.
//  relaxation   fl(a + w) is monotone in a, and a + w >= a for w >= 0.  Starting from dist = +inf, dist[source] = 0, the kernel
//               repeats  dist[v] <- min(dist[v], fl(dist[u] + w(u, v)))  in any order until a sweep changes nothing:
//                 1 every value written is the sum along a realised path, so it is at least the answer;
//                 2 at termination, induction along an optimal path (its prefix is optimal up to equal sums: monotonicity) gives
//                   dist[v] <= fl(dist[u] + w) <= the path's sum, so it is at most the answer;
//                 3 so the two are equal, whatever the order, and a stale read of a neighbour (a value written earlier) is allowed.
//               A value never rises along a path, so a candidate above max_dist cannot lie on a path to a value at or below it:
//               the kernel drops such candidates, and the reported bits are those of thresholding the uncapped field.
//               Like Bellman-Ford, sweep k has settled every vertex whose optimal path has at most k edges: V - 1 sweeps settle
//               all, one more sees no change, and the kernel's loop ends at V sweeps whatever happens.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace smplpp_hip
{
constexpr int64_t GEO_MAX_V = 32768;           // the field of one (frame, source set) lives in LDS: V floats
constexpr int64_t GEO_LDS_FLAGS = 16;          // bytes after the field: the three changed flags of the sweeps (and padding)
constexpr int64_t GEO_LDS_STATIC = 64 * 1024;  // above this many bytes a kernel opts in to its LDS (common.h, lds_opt_in)
constexpr int64_t GEO_LDS_MAX = 160 * 1024;    // LDS of a gfx950 workgroup
constexpr int GEO_THREADS = 1024;              // threads of the relaxation's workgroup
constexpr int64_t GEO_INT32_MAX = 0x7fffffffLL;

// The undirected edge set of [F,3] faces as a per-vertex CSR: the neighbours of v are adj[off[v] .. off[v+1]), ascending, each once,
// never v itself.  Faces may repeat, share an edge among more than two of them, or name a vertex twice; a vertex in no face has an
// empty row.  src[e] is the row of entry e (the kernel that writes the edge lengths takes one thread per entry).
struct EdgeTable
{
  const char * refusal = nullptr; // why the table is refused, or null
  int64_t V = 0, nnz = 0;         // nnz = 2 * (undirected edges)
  std::vector<int32_t> off;       // [V+1]
  std::vector<int32_t> adj;       // [nnz]
  std::vector<int32_t> src;       // [nnz]
};

// faces: [F][3] 0-based int32 host array
inline EdgeTable edge_table(int64_t V, int64_t F, const int32_t * faces)
{
  EdgeTable t;
  if(V <= 0 || V > GEO_INT32_MAX) return t.refusal = "V must be in [1, 2^31)", t;
  if(F <= 0) return t.refusal = "the model has no faces", t;
  if(F > GEO_INT32_MAX / 6) return t.refusal = "F beyond int32 indexing", t;
  if(!faces) return t.refusal = "faces is NULL", t;
  for(int64_t i = 0; i < F * 3; i++)
    if(faces[i] < 0 || faces[i] >= V) return t.refusal = "a face corner is outside [0, V)", t;
  // every directed pair (a, b), a != b, as one 64-bit key; sorted and made unique, the keys are the CSR in order
  std::vector<uint64_t> key;
  key.reserve((size_t)F * 6);
  for(int64_t f = 0; f < F; f++)
    for(int c = 0; c < 3; c++)
    {
      const uint64_t a = (uint64_t)faces[f * 3 + c], b = (uint64_t)faces[f * 3 + (c + 1) % 3];
      if(a == b) continue;
      key.push_back(a << 32 | b);
      key.push_back(b << 32 | a);
    }
  std::sort(key.begin(), key.end());
  key.erase(std::unique(key.begin(), key.end()), key.end());
  t.V = V, t.nnz = (int64_t)key.size();
  t.off.assign((size_t)V + 1, 0);
  t.adj.resize(key.size());
  t.src.resize(key.size());
  for(size_t e = 0; e < key.size(); e++)
  {
    t.src[e] = (int32_t)(key[e] >> 32);
    t.adj[e] = (int32_t)(key[e] & 0xffffffffu);
    t.off[(size_t)t.src[e] + 1]++;
  }
  for(int64_t v = 0; v < V; v++) t.off[(size_t)v + 1] += t.off[(size_t)v];
  return t;
}

// The launch of the relaxation for a model of V vertices
struct GeodesicPlan
{
  const char * refusal = nullptr;
  int64_t lds_bytes = 0;   // the field, V floats, and GEO_LDS_FLAGS bytes of flags after it: all of the workgroup's LDS
  bool opt_in = false;     // lds_bytes is above what a kernel gets without asking (64 KiB: from V = 16381 on)
  int64_t max_sweeps = 0;  // the loop's bound: V (V - 1 settle every vertex, one more sees no change)
};

inline GeodesicPlan geodesic_plan(int64_t V)
{
  GeodesicPlan p;
  if(V <= 0) return p.refusal = "V must be positive", p;
  if(V > GEO_MAX_V) return p.refusal = "V above 32768: the field does not fit in LDS", p;
  p.lds_bytes = V * (int64_t)sizeof(float) + GEO_LDS_FLAGS;
  p.opt_in = p.lds_bytes > GEO_LDS_STATIC;
  p.max_sweeps = V;
  return p;
}

// source_ptr [S+1], source_vertex [source_ptr[S]] host arrays (source_vertex null: a device-space call, its ids are not read here)
inline const char * geodesic_sources_refusal(int64_t V, int64_t S, const int64_t * source_ptr, const int64_t * source_vertex)
{
  if(S <= 0) return "S must be positive";
  if(!source_ptr) return "source_ptr is NULL";
  if(source_ptr[0] != 0) return "source_ptr[0] must be 0";
  for(int64_t s = 0; s < S; s++)
    if(source_ptr[s + 1] < source_ptr[s]) return "source_ptr must be non-decreasing";
  if(source_ptr[S] > GEO_INT32_MAX) return "the source list is beyond int32 indexing";
  if(source_vertex)
    for(int64_t e = 0; e < source_ptr[S]; e++)
      if(source_vertex[e] < 0 || source_vertex[e] >= V) return "a source vertex is outside [0, V)";
  return nullptr;
}

// words per row of the far mask [V][W]
inline int64_t contact_mask_words(int64_t V)
{
  return (V + 31) / 32;
}
} // namespace smplpp_hip
