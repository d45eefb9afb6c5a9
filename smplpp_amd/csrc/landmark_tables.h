// The host tables of a landmark regressor: what smplpp_landmarks_create (landmarks.hip) computes from the caller's CSR before it
// uploads anything.  Plain C++17, no HIP: a CPU test runs the builder as a stand-alone program (tests/cpp/landmark_tables_dump.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace smplpp_hip
{
constexpr int64_t LM_MAX_ROWS = 65535;
constexpr int64_t LM_INT32_MAX = 0x7fffffffLL;

// The regressor as the kernels read it: the CSR with int32 columns (forward), and its transpose (backward): per source column s the
// entries e that name it, in ascending e, as (landmark row, weight)
struct LandmarkTables
{
  const char * refusal = nullptr; // why the regressor is refused, or null
  int64_t L = 0, nnz = 0, S = 0;  // rows, entries, source columns (V + 24)
  std::vector<int32_t> rowPtr;    // [L+1]
  std::vector<int32_t> col;       // [nnz]
  std::vector<float> val;         // [nnz]
  std::vector<int32_t> srcPtr;    // [S+1]
  std::vector<int32_t> srcRow;    // [nnz] row l of the entry
  std::vector<float> srcVal;      // [nnz]
};

// S = V + 24 source columns; row_ptr [L+1], col and val [row_ptr[L]] host arrays
inline LandmarkTables landmark_tables(int64_t L, int64_t S, const int64_t * row_ptr, const int64_t * col, const float * val)
{
  LandmarkTables t;
  if(L < 1 || L > LM_MAX_ROWS) return t.refusal = "L must be in [1, 65535]", t;
  if(S < 1 || S > LM_INT32_MAX) return t.refusal = "V + 24 beyond int32 indexing", t;
  if(!row_ptr) return t.refusal = "row_ptr is NULL", t;
  if(row_ptr[0] != 0) return t.refusal = "row_ptr[0] must be 0", t;
  for(int64_t l = 0; l < L; l++)
    if(row_ptr[l + 1] < row_ptr[l]) return t.refusal = "row_ptr must be non-decreasing", t;
  const int64_t nnz = row_ptr[L];
  if(nnz > LM_INT32_MAX) return t.refusal = "nnz beyond int32 indexing", t;
  if(nnz > 0 && (!col || !val)) return t.refusal = "col or val is NULL", t;
  for(int64_t e = 0; e < nnz; e++)
  {
    if(col[e] < 0 || col[e] >= S) return t.refusal = "a column is outside [0, V + 24)", t;
    if(!std::isfinite(val[e])) return t.refusal = "a val is not finite", t;
  }
  t.L = L, t.nnz = nnz, t.S = S;
  t.rowPtr.assign(row_ptr, row_ptr + L + 1);
  t.col.assign(col, col + nnz);
  t.val.assign(val, val + nnz);
  // the transpose by a counting sort over e, which keeps every source's entries in ascending e
  t.srcPtr.assign((size_t)S + 1, 0);
  for(int64_t e = 0; e < nnz; e++) t.srcPtr[(size_t)col[e] + 1]++;
  for(int64_t s = 0; s < S; s++) t.srcPtr[(size_t)s + 1] += t.srcPtr[(size_t)s];
  t.srcRow.resize((size_t)nnz);
  t.srcVal.resize((size_t)nnz);
  std::vector<int32_t> next(t.srcPtr.begin(), t.srcPtr.end() - 1);
  for(int64_t l = 0; l < L; l++)
    for(int64_t e = row_ptr[l]; e < row_ptr[l + 1]; e++)
    {
      const int32_t q = next[(size_t)col[e]]++;
      t.srcRow[(size_t)q] = (int32_t)l;
      t.srcVal[(size_t)q] = val[e];
    }
  return t;
}
} // namespace smplpp_hip
