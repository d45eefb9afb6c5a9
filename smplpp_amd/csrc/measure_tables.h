// The host tables of a measurement handle: what smplpp_measure_create (measure.hip) computes from the caller's regions and sections
// before it uploads anything.  Plain C++17, no HIP: a CPU test runs the builder as a stand-alone program
// (tests/cpp/measure_tables_dump.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace smplpp_hip
{
constexpr int64_t MS_MAX_REGIONS = 256;
constexpr int64_t MS_MAX_SECTIONS = 256;
constexpr int64_t MS_INT32_MAX = 0x7fffffffLL;

// The regions and sections as the kernels read them: the region lists with int32 face ids (forward, and the backward to the planes);
// per face the (region, slot) pairs that hold it, in ascending region (backward to the vertices); per region its sections in
// ascending s (both).
struct MeasureTables
{
  const char * refusal = nullptr;   // why the handle is refused, or null
  int64_t R = 0, nnz = 0, S = 0, F = 0;
  std::vector<int32_t> regionPtr;   // [R+1]
  std::vector<int32_t> regionFace;  // [nnz] face of slot k of region r at regionPtr[r] + k
  std::vector<int32_t> facePtr;     // [F+1]
  std::vector<int32_t> faceRegion;  // [nnz] the regions that list the face, ascending
  std::vector<int32_t> faceSlot;    // [nnz] the face's slot k in that region's list
  std::vector<int32_t> secPtr;      // [R+1]
  std::vector<int32_t> secId;       // [S] the sections of region r, ascending s
  std::vector<int32_t> secRegion;   // [S] the caller's section_region
};

// F faces in the model; region_ptr [R+1], region_face [region_ptr[R]], section_region [S] host arrays
inline MeasureTables measure_tables(int64_t F, int64_t R, const int64_t * region_ptr, const int64_t * region_face, int64_t S,
                                    const int64_t * section_region)
{
  MeasureTables t;
  if(F < 0 || F > MS_INT32_MAX) return t.refusal = "F beyond int32 indexing", t;
  if(R < 1 || R > MS_MAX_REGIONS) return t.refusal = "R must be in [1, 256]", t;
  if(S < 0 || S > MS_MAX_SECTIONS) return t.refusal = "S must be in [0, 256]", t;
  if(!region_ptr) return t.refusal = "region_ptr is NULL", t;
  if(region_ptr[0] != 0) return t.refusal = "region_ptr[0] must be 0", t;
  for(int64_t r = 0; r < R; r++)
    if(region_ptr[r + 1] < region_ptr[r]) return t.refusal = "region_ptr must be non-decreasing", t;
  const int64_t nnz = region_ptr[R];
  if(nnz > MS_INT32_MAX) return t.refusal = "nnz beyond int32 indexing", t;
  if(nnz > 0 && !region_face) return t.refusal = "region_face is NULL", t;
  if(S > 0 && !section_region) return t.refusal = "section_region is NULL", t;
  for(int64_t e = 0; e < nnz; e++)
    if(region_face[e] < 0 || region_face[e] >= F) return t.refusal = "a face id is outside [0, F)", t;
  for(int64_t s = 0; s < S; s++)
    if(section_region[s] < 0 || section_region[s] >= R) return t.refusal = "a section_region is outside [0, R)", t;
  // a face at most once in a region: the last region that listed it, per face
  std::vector<int32_t> seen((size_t)F, -1);
  for(int64_t r = 0; r < R; r++)
    for(int64_t e = region_ptr[r]; e < region_ptr[r + 1]; e++)
    {
      int32_t & last = seen[(size_t)region_face[e]];
      if(last == (int32_t)r) return t.refusal = "a face is listed twice in a region", t;
      last = (int32_t)r;
    }
  t.R = R, t.nnz = nnz, t.S = S, t.F = F;
  t.regionPtr.assign(region_ptr, region_ptr + R + 1);
  t.regionFace.assign(region_face, region_face + nnz);
  // the transpose by a counting sort over the regions in ascending r, which keeps every face's pairs in ascending region
  t.facePtr.assign((size_t)F + 1, 0);
  for(int64_t e = 0; e < nnz; e++) t.facePtr[(size_t)region_face[e] + 1]++;
  for(int64_t f = 0; f < F; f++) t.facePtr[(size_t)f + 1] += t.facePtr[(size_t)f];
  t.faceRegion.resize((size_t)nnz);
  t.faceSlot.resize((size_t)nnz);
  std::vector<int32_t> next(t.facePtr.begin(), t.facePtr.end() - 1);
  for(int64_t r = 0; r < R; r++)
    for(int64_t e = region_ptr[r]; e < region_ptr[r + 1]; e++)
    {
      const int32_t q = next[(size_t)region_face[e]]++;
      t.faceRegion[(size_t)q] = (int32_t)r;
      t.faceSlot[(size_t)q] = (int32_t)(e - region_ptr[r]);
    }
  // the sections of every region, ascending s
  t.secPtr.assign((size_t)R + 1, 0);
  for(int64_t s = 0; s < S; s++) t.secPtr[(size_t)section_region[s] + 1]++;
  for(int64_t r = 0; r < R; r++) t.secPtr[(size_t)r + 1] += t.secPtr[(size_t)r];
  t.secId.resize((size_t)S);
  t.secRegion.resize((size_t)S);
  std::vector<int32_t> nexts(t.secPtr.begin(), t.secPtr.end() - 1);
  for(int64_t s = 0; s < S; s++)
  {
    t.secId[(size_t)nexts[(size_t)section_region[s]]++] = (int32_t)s;
    t.secRegion[(size_t)s] = (int32_t)section_region[s];
  }
  return t;
}
} // namespace smplpp_hip
