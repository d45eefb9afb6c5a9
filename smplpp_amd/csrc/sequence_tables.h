// The host tables of a sequence layout: what smplpp_sequence_create (sequence.hip) computes from the optimiser's grouping
// before it uploads anything.  Problem p owns the rows row_start[p] .. row_start[p+1]-1 of the optimiser buffer; its last shared_rows
// rows are not frames; the frames of all problems are numbered compactly in row order.  Plain C++17, no HIP: a CPU test runs the builder
// as a stand-alone program (tests/cpp/sequence_tables_dump.cpp).  What is refused for row_start is what smplpp_lbfgs_create_grouped
// refuses (lbfgs_wide_plan.h).
#pragma once

#include <cstdint>
#include <vector>

#include "lbfgs_wide_plan.h"

namespace smplpp_hip
{
constexpr int64_t SEQ_INT32_MAX = 0x7fffffffLL;

struct SequenceTables
{
  const char * refusal = nullptr; // why the layout is refused, or null
  int64_t P = 0, rows = 0, frames = 0;
  int shared_rows = 0;
  std::vector<int64_t> row_start;   // [P+1] as given
  std::vector<int64_t> frame_start; // [P+1]: problem p owns the frames frame_start[p] .. frame_start[p+1]-1
  std::vector<int32_t> problem_of;  // [F] the problem of a frame
  std::vector<int32_t> row_of;      // [F] the row of a frame in the optimiser buffer
  std::vector<int32_t> frame_of;    // [rows] the frame of a row, or -1 - p for the shared row of problem p
};

inline SequenceTables sequence_tables(int64_t P, const int64_t * row_start, int shared_rows)
{
  SequenceTables t;
  if(P <= 0) return t.refusal = "P must be positive", t;
  if(!row_start) return t.refusal = "row_start is NULL", t;
  if(const char * why = lbfgs_groups_refusal(row_start[P], P, row_start)) return t.refusal = why, t;
  if(shared_rows != 0 && shared_rows != 1) return t.refusal = "shared_rows must be 0 or 1", t;
  if(row_start[P] > SEQ_INT32_MAX) return t.refusal = "rows beyond int32 indexing", t;
  for(int64_t p = 0; p < P; p++)
    if(row_start[p + 1] - row_start[p] - shared_rows < 1) return t.refusal = "a problem has no frame beside its shared row", t;
  t.P = P, t.rows = row_start[P], t.shared_rows = shared_rows, t.frames = t.rows - P * shared_rows;
  t.row_start.assign(row_start, row_start + P + 1);
  t.frame_start.resize((size_t)(P + 1));
  t.problem_of.resize((size_t)t.frames);
  t.row_of.resize((size_t)t.frames);
  t.frame_of.resize((size_t)t.rows);
  int64_t f = 0;
  for(int64_t p = 0; p < P; p++)
  {
    t.frame_start[(size_t)p] = f;
    const int64_t T = row_start[p + 1] - row_start[p] - shared_rows;
    for(int64_t j = 0; j < T; j++, f++)
      t.problem_of[(size_t)f] = (int32_t)p, t.row_of[(size_t)f] = (int32_t)(row_start[p] + j), t.frame_of[(size_t)(row_start[p] + j)] = (int32_t)f;
    if(shared_rows) t.frame_of[(size_t)(row_start[p + 1] - 1)] = (int32_t)(-1 - p);
  }
  t.frame_start[(size_t)P] = f;
  return t;
}
} // namespace smplpp_hip
