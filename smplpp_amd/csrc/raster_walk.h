// What the backward passes of the image-space terms share: the rasteriser's per-handle state, its vertex pass,
// the walk of a face's clipped box by DR_SPLIT lanes, and the gather of the per-face sums to the vertices.  The pieces of the rule
// are in depth_raster_device.h; the vertex pass and the gather are defined once, in depth_raster.hip.
#pragma once
#include "depth_raster_device.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int DR_T = 256;     // threads of every kernel of depth_raster.hip and raster_interpolate.hip
constexpr int DR_SPLIT = 8;   // lanes per face in the backward walk

// One per handle, grown to the largest call: scratch of whichever image-space call is in flight on the handle.
struct DepthRasterState
{
  DevBuf cam, snap;   // [n][V] float4 camera-space vertex, int2 snapped projection
  DevBuf keys;        // [n][H][W] uint64
  DevBuf queue, qn;   // [n][F] int32 queued (frame, face) items and their count
  DevBuf fsum;        // [n][F][row] per-face corner sums of the backward walk in flight (row = 9 depth, 12 interpolation)
  int inline_px = 0;   // box pixels a face's own thread walks in the forward (set by dr_state)
};
DepthRasterState * dr_state(smplpp_model * m);

inline unsigned dr_grid(int64_t items)
{
  return (unsigned)((items + DR_T - 1) / DR_T);
}

// s->cam, s->snap of n frames (dr_vertex_kernel); all pointers on the device
int dr_vertex_pass(smplpp_model * m, DepthRasterState * s, int64_t n, const float * verts, const float * camera, float near, hipStream_t st);

// out[(frame V + v) stride + off + x], x < width, width in 1 .. 4: the sum over the vertex's faces, in ascending face id, then corner,
// each from +0, of fsum[(frame F + face) row + corner width + x]; with rot (width 3), R^T of camera first (dr_gather_kernel)
int dr_gather(smplpp_model * m, int64_t n, const float * fsum, int row, int width, bool rot, const float * camera, float * out,
              int stride, int off, int accumulate, hipStream_t st);

// The (frame, face) of this thread and its share of the face's box
struct DrWalk
{
  int64_t idx, frame, f; // idx = frame F + f
  int part;              // lane of the face, 0 .. DR_SPLIT - 1
  bool in, live;         // idx < nf; the face has a box to walk (t is set)
  DrFace t;
};

// The backward walk of every image-space term, for a grid of dr_grid(nf * DR_SPLIT) blocks of DR_T threads: DR_SPLIT consecutive
// lanes take one (frame, face); the face's clipped box is walked in row-major order, lane l taking entries l, l + DR_SPLIT, ...; a
// pixel whose face id is the face's goes to body.pixel, which adds to the lane's N running sums s; then the lanes' sums meet in a
// fixed xor tree, ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7)), so every lane of the face holds the total.  body.face runs once before the
// pixels of a live face.  Every thread of the grid must call this (the tree takes the lanes of faces that are not live, with zeros);
// the caller stores from the lane with in && part == 0.
template<int N, class Body>
__device__ inline DrWalk dr_walk(const float4 * __restrict__ cam, const int2 * __restrict__ snap, const int32_t * __restrict__ faces,
                                 const int64_t * __restrict__ face, int64_t H, int64_t W, int64_t V, int64_t F, int64_t nf,
                                 float (&s)[N], Body & body)
{
  DrWalk w;
  const int64_t tid = (int64_t)blockIdx.x * DR_T + threadIdx.x;
  w.idx = tid / DR_SPLIT;
  w.part = (int)(tid % DR_SPLIT);
  w.in = w.idx < nf;
  w.frame = w.in ? w.idx / F : 0, w.f = w.in ? w.idx % F : 0;
  w.live = w.in && dr_face_setup(w.t, cam, snap, faces, w.frame, w.f, V, H, W) == DR_FACE_OK;
#pragma unroll
  for(int k = 0; k < N; k++) s[k] = 0.0f;
  if(w.live)
  {
    body.face(w.t, w.frame, w.f);
    const int64_t * ff = face + w.frame * H * W;
    const int bw = w.t.i1 - w.t.i0 + 1;
    const int64_t area = (int64_t)bw * (w.t.j1 - w.t.j0 + 1);
    for(int64_t r = w.part; r < area; r += DR_SPLIT)
    {
      const int i = w.t.i0 + (int)(r % bw), j = w.t.j0 + (int)(r / bw);
      const int64_t pix = (int64_t)j * W + i;
      if(ff[pix] != w.f) continue;
      body.pixel(w.t, i, j, pix, s);
    }
  }
  for(int m = DR_SPLIT / 2; m >= 1; m >>= 1)
#pragma unroll
    for(int k = 0; k < N; k++) s[k] = s[k] + __shfl_xor(s[k], m);
  return w;
}
} // namespace smplpp_hip
