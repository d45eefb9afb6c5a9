// The host tables of a model: what smplpp_model_create (model.hip) computes from the model's arrays before it uploads anything.
// One function per table family; each takes host arrays and returns host vectors.  Plain C++17, no HIP: a CPU test runs every
// function here as a stand-alone program (tests/cpp/model_tables_dump.cpp).  Layouts: layout.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "layout.h"

namespace smplpp_hip
{
// Each check returns why the model is refused, or null.
// kinematic tree: row 0 = parent (src/WorldTransformation.cpp:523); must be topologically ordered like SMPL's
inline const char * check_tree(const int64_t * kintree, std::vector<int32_t> & parent)
{
  parent.assign(NJ, -1);
  for(int i = 1; i < NJ; i++)
  {
    if(kintree[i] < 0 || kintree[i] >= i) return "Cannot set kinematic tree: parent(i) must precede i";
    parent[i] = (int32_t)kintree[i];
  }
  return nullptr;
}
inline const char * check_faces(const int32_t * faces1, int64_t F, int64_t V)
{
  for(int64_t i = 0; i < F * 3; i++)
    if(faces1[i] < 1 || faces1[i] > V) return "face_indices must be 1-based vertex ids";
  return nullptr;
}

// Skinning weights: the non-zeros are kept (real SMPL has <= 4 per vertex), a dense table otherwise.
struct SkinWeights
{
  int maxw = 0;              // weights kept per vertex: 4, 8 or 24
  std::vector<uint8_t> wIdx; // [VGn*32][maxw] joints, ascending
  std::vector<float> wVal;   // [VGn*32][maxw]
  std::vector<float> wSum;   // [VGn*32] sum_j W[v,j] (rows past V: 1)
};
inline SkinWeights skin_weights(const float * W, int64_t V)
{
  int maxnz = 0;
  for(int64_t v = 0; v < V; v++)
  {
    int nz = 0;
    for(int j = 0; j < NJ; j++) nz += (W[v * NJ + j] != 0.0f);
    maxnz = std::max(maxnz, nz);
  }
  SkinWeights t;
  t.maxw = maxnz <= 4 ? 4 : (maxnz <= 8 ? 8 : NJ);
  const int64_t Vpad = (V + VG - 1) / VG * VG;
  t.wIdx.assign((size_t)Vpad * t.maxw, 0);
  t.wVal.assign((size_t)Vpad * t.maxw, 0.0f);
  t.wSum.assign((size_t)Vpad, 1.0f);
  for(int64_t v = 0; v < V; v++)
  {
    int q = 0;
    float s = 0.0f;
    for(int j = 0; j < NJ; j++)
    {
      float w = W[v * NJ + j];
      s += w; // ascending j, fp32: h[3] = sum_j W[v,j] * 1 (src/LinearBlendSkinning.cpp:463-467)
      if(t.maxw == NJ)
      {
        t.wIdx[v * NJ + j] = (uint8_t)j;
        t.wVal[v * NJ + j] = w;
      }
      else if(w != 0.0f)
      {
        t.wIdx[v * t.maxw + q] = (uint8_t)j;
        t.wVal[v * t.maxw + q] = w;
        q++;
      }
    }
    t.wSum[v] = s;
  }
  return t;
}

// fp16x2 operands: power-of-two scales that put the largest basis entry / a generous bound of the relative
// translations (16 x the template's extent) just under fp16's range, so that both pieces of every value that matters
// are normal fp16 numbers
struct HScales
{
  float sB = 1.0f, sG = 1.0f;
  const char * refusal = nullptr; // the bases and the template are all zero, or hold a value that is not finite
};
inline HScales h_scales(const float * P, const float * S, const float * vt, int64_t V)
{
  HScales t;
  float bmax = 0.0f, tmax = 0.0f;
  for(int64_t i = 0; i < V * 3 * NP; i++) bmax = std::max(bmax, std::fabs(P[i]));
  for(int64_t i = 0; i < V * 3 * NB; i++) bmax = std::max(bmax, std::fabs(S[i]));
  for(int64_t i = 0; i < V * 3; i++) tmax = std::max(tmax, std::fabs(vt[i]));
  bmax = std::max(bmax, tmax);
  if(!(bmax > 0.0f) || !std::isfinite(bmax))
  {
    t.refusal = "Cannot initialize a SMPL model!";
    return t;
  }
  t.sB = std::exp2(std::floor(std::log2(32768.0f / bmax)));
  t.sG = std::exp2(std::floor(std::log2(32768.0f / (16.0f * tmax > 1.0f ? 16.0f * tmax : 1.0f))));
  return t;
}

// Vertex groups of the h form by skinning class (layout.h, HB_PERM_OFF).  (1) A group is 64 CONSECUTIVE vertices and its class what
// their weights touch — joints 0..15 only, both halves, joints 16..23 only.  (Sorting the VERTICES by class first, which makes 73 of
// the synthetic model's 108 groups single-class instead of 11, was measured: the step went from 46 to 62 us — a group's 64
// output rows of 12 bytes were then scattered over ~200 vertex positions, and the 85 MB of write-once output lost its
// coalescing.  Models whose vertex order follows the body parts — SMPL's does — have their single-class groups as they are.)
// (2) the groups dealt round-robin over the eight XCD slices of skin_kernel_h ([x nvg / 8, (x + 1) nvg / 8)), so that every XCD
// gets the same mix; (3) inside a slice the classes interleaved by fractional rank, so that every workgroup's run of
// consecutive groups gets it too (a slice of cheap groups beside a slice of full ones would finish with the full ones).
struct VertexGroups
{
  std::vector<int32_t> perm;  // [nvg * 64] the vertex in each slot of each group (-1: none)
  std::vector<int32_t> flags; // [nvg] bit 0: the group has a weight on joints 0..15, bit 1: on joints 16..23
};
inline VertexGroups h_vertex_groups(const float * W, int64_t V)
{
  const int64_t nvg = (V + 63) / 64;
  VertexGroups t;
  t.perm.assign((size_t)nvg * 64, -1);
  t.flags.assign((size_t)nvg, 1);
  std::vector<int> tflags((size_t)nvg, 0); // flags of the groups in vertex order
  for(int64_t v = 0; v < V; v++)
  {
    bool lo = false, hi = false;
    for(int j = 0; j < NJ; j++)
      if(W[v * NJ + j] != 0.0f) (j < 16 ? lo : hi) = true;
    tflags[(size_t)(v / 64)] |= hi ? (lo ? 3 : 2) : 1;
  }
  // (2) + (3): per XCD slice the groups it is dealt, then their order inside the slice
  std::vector<std::vector<int64_t>> bin(8);
  {
    int x = 0;
    for(int64_t g = 0; g < nvg; g++)
    {
      for(int tries = 0; tries < 8 && (int64_t)bin[x].size() >= (((x + 1) * nvg) >> 3) - ((x * nvg) >> 3); tries++) x = (x + 1) & 7;
      bin[x].push_back(g);
      x = (x + 1) & 7;
    }
  }
  int64_t g = 0;
  for(int x = 0; x < 8; x++)
  {
    int cnt[4] = {0, 0, 0, 0}, seen[4] = {0, 0, 0, 0};
    for(int64_t s : bin[x]) cnt[tflags[(size_t)s]]++;
    std::vector<std::pair<double, int64_t>> keyed;
    for(int64_t s : bin[x])
    {
      const int f = tflags[(size_t)s];
      keyed.push_back({(seen[f] + 0.5) / cnt[f], s});
      seen[f]++;
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<double, int64_t> & a, const std::pair<double, int64_t> & b) { return a.first < b.first; });
    for(auto & ks : keyed)
    {
      const int64_t s = ks.second;
      for(int i = 0; i < 64 && s * 64 + i < V; i++) t.perm[(size_t)(g * 64 + i)] = (int32_t)(s * 64 + i);
      t.flags[(size_t)g] = tflags[(size_t)s] ? tflags[(size_t)s] : 1;
      g++;
    }
  }
  return t;
}

// Joints by depth: the FK chain advances one tree level per step (SMPL: 9 levels)
struct JointLevels
{
  std::vector<int32_t> depth; // [24]
  int nlev = 1;
};
inline JointLevels joint_levels(const std::vector<int32_t> & parent)
{
  JointLevels t;
  t.depth.assign(NJ, 0);
  for(int i = 1; i < NJ; i++)
  {
    t.depth[i] = t.depth[parent[i]] + 1;
    t.nlev = std::max(t.nlev, t.depth[i] + 1);
  }
  return t;
}

// smplpp_model::lvl: level offsets, joints by level, and from CT_OFF, per (level, slot), the joint and its parent for the pose
// kernel's chain wavefront (5 joints of a level at a time, 12 lanes each): read once into registers instead of three dependent LDS
// look-ups per level.  chain_fast: the tree has at most CT_LEV levels of at most 5 joints (SMPL: 9 levels, widest 5); other trees
// take the generic loop.
struct ChainTables
{
  std::vector<int32_t> lvl; // [CT_OFF + 60 CT_LEV 2]
  bool chain_fast = false;
};
inline ChainTables chain_tables(const std::vector<int32_t> & parent, const JointLevels & levels)
{
  const int nlev = levels.nlev;
  ChainTables t;
  std::vector<int32_t> & lv = t.lvl;
  lv.assign(CT_OFF + 60 * CT_LEV * 2, 0);
  int pos = 0;
  for(int L = 0; L < nlev; L++)
  {
    lv[L] = pos;
    for(int i = 0; i < NJ; i++)
      if(levels.depth[i] == L) lv[NJ + 1 + pos++] = i;
  }
  lv[nlev] = pos;
  t.chain_fast = nlev <= CT_LEV;
  for(int q = 0; q < 60 * CT_LEV; q++)
  {
    lv[CT_OFF + 2 * q] = 0x00ffff;
    lv[CT_OFF + 2 * q + 1] = CT_P_ZERO | (CT_P_ZERO << 10) | (1 << 20);
  }
  std::vector<int> slot_of(NJ, 0); // slot of a joint inside its level
  for(int L = 0; L < nlev && t.chain_fast; L++)
  {
    const int cnt = lv[L + 1] - lv[L];
    if(cnt > 5) t.chain_fast = false;
    for(int q = 0; q < cnt && q < 5; q++)
    {
      const int i = lv[NJ + 1 + lv[L] + q];
      slot_of[i] = q;
      const int p = parent[i];
      const int word = i | ((p >= 0 ? p : 0xff) << 8) | ((p >= 0 ? slot_of[p] : 0) << 16); // (the parent sits one level up: already placed)
      for(int e = 0; e < 12; e++)
      {
        const int c = e % 4;
        // the lane's operand: column c of R_i (stride 3), or j_i minus j_p (root: minus zero)
        const int aidx = c < 3 ? CT_P_R + i * 9 + c : CT_P_J + i * 3;
        const int bidx = (c == 3 && p >= 0) ? CT_P_J + p * 3 : CT_P_ZERO;
        lv[CT_OFF + ((q * 12 + e) * CT_LEV + L) * 2] = word;
        lv[CT_OFF + ((q * 12 + e) * CT_LEV + L) * 2 + 1] = aidx | (bidx << 10) | ((c < 3 ? 3 : 1) << 20);
      }
    }
  }
  return t;
}

// smplpp_model::anc, the tree tables of the IK evaluation (layout.h, TREE_*); trees deeper than TREE_DMAX keep the masks only
// (smplpp_ik_create refuses them)
inline std::vector<int32_t> ik_tree_tables(const std::vector<int32_t> & parent, const JointLevels & levels)
{
  std::vector<int32_t> tr(TREE_SIZE, -1);
  for(int i = 0; i < NJ; i++) tr[TREE_ANC + i] = (1 << i) | (i ? tr[TREE_ANC + parent[i]] : 0);
  int pos = 0;
  for(int L = 0; L <= TREE_DMAX; L++)
  {
    tr[TREE_LVL + L] = pos;
    for(int i = 0; i < NJ && L < TREE_DMAX; i++)
      if(levels.depth[i] == L) tr[TREE_LVLJ + pos++] = i;
  }
  return tr;
}

// Faces and the per-vertex adjacent-face table (src/SMPL.cpp:620-640; emplace keeps one entry per (vertex, face))
struct Adjacency
{
  std::vector<int32_t> faces;   // [F][3] 0-based
  std::vector<int32_t> adjOff;  // [V + 1]
  std::vector<int32_t> adjFace; // [adjOff[V]] ascending face id per vertex
};
inline Adjacency adjacency(const int32_t * faces1, int64_t F, int64_t V)
{
  Adjacency t;
  t.faces.resize((size_t)F * 3);
  for(int64_t i = 0; i < F * 3; i++) t.faces[i] = faces1[i] - 1;
  std::vector<std::vector<int32_t>> adj((size_t)V);
  for(int64_t f = 0; f < F; f++)
    for(int i = 0; i < 3; i++)
    {
      auto & a = adj[t.faces[f * 3 + i]];
      if(a.empty() || a.back() != (int32_t)f) a.push_back((int32_t)f);
    }
  t.adjOff.assign((size_t)V + 1, 0);
  for(int64_t v = 0; v < V; v++) t.adjOff[v + 1] = t.adjOff[v] + (int32_t)adj[v].size();
  t.adjFace.reserve((size_t)t.adjOff[V]);
  for(int64_t v = 0; v < V; v++) t.adjFace.insert(t.adjFace.end(), adj[v].begin(), adj[v].end());
  return t;
}

// IK ring tables (topology only): what a task on face f touches when it differentiates a normal — the face's vertices
// (slots 0..2), then the distinct vertices of the faces around them, first occurrence first; the map gives every
// (vertex of the face, adjacent face, corner) its slot.  The tables hold `madj` faces per vertex: 12, or 16 when some vertex of
// this topology has more (the evaluation then runs its 16-face instantiation; beyond 16 a task with a normal term on such a
// vertex is reported, smplpp_ik_get_status bit 2) — and 3 (madj + 1) + 1 ring vertices.  No tables (and madj = MAXADJ) for a mesh
// without faces or with more vertices than a ring entry's 16 bits hold.
struct RingTables
{
  int madj = MAXADJ;
  std::vector<uint16_t> faceRing; // [F][3 (madj + 1) + 2] count, then the ring
  std::vector<uint8_t> faceMap;   // [F][3 madj 3]
};
inline RingTables ik_ring_tables(const int32_t * faces, const int32_t * adjOff, const int32_t * adjFace, int64_t F, int64_t V)
{
  RingTables t;
  if(V > 65535 || F <= 0) return t;
  int maxval = 0;
  for(int64_t v = 0; v < V; v++) maxval = std::max<int>(maxval, adjOff[v + 1] - adjOff[v]);
  t.madj = maxval > MAXADJ ? MAXADJ_WIDE : MAXADJ;
  const int MADJ_ = t.madj, MRING_ = 3 * (MADJ_ + 1) + 1;
  t.faceRing.assign((size_t)F * (MRING_ + 1), 0);
  t.faceMap.assign((size_t)F * 3 * MADJ_ * 3, 0);
  for(int64_t f = 0; f < F; f++)
  {
    uint16_t * rg = t.faceRing.data() + f * (MRING_ + 1);
    uint8_t * mp = t.faceMap.data() + f * (3 * MADJ_ * 3);
    int nr = 0;
    for(int i = 0; i < 3; i++) rg[1 + nr++] = (uint16_t)faces[f * 3 + i];
    for(int i = 0; i < 3; i++)
    {
      const int32_t u = faces[f * 3 + i], b0 = adjOff[u];
      const int cnt = std::min<int>(adjOff[u + 1] - b0, MADJ_);
      for(int a = 0; a < cnt; a++)
        for(int cc = 0; cc < 3; cc++)
        {
          const int32_t v = faces[(int64_t)adjFace[b0 + a] * 3 + cc];
          int slot = -1;
          for(int q = 0; q < nr; q++)
            if(rg[1 + q] == (uint16_t)v) slot = q;
          if(slot < 0 && nr < MRING_)
          {
            slot = nr;
            rg[1 + nr++] = (uint16_t)v;
          }
          mp[(i * MADJ_ + a) * 3 + cc] = (uint8_t)(slot < 0 ? 0 : slot);
        }
    }
    rg[0] = (uint16_t)nr;
  }
  return t;
}

// Forms of the fused kernel, {smplpp_fk's, the IK / VPoser loops' internal launches'}, decided once at model creation.  Default:
// smplpp_fk runs e (skin_e.hip: fp32-exact operands, the reference's arithmetic) and the loops h (skin_h.hip: fp16x2 operands,
// 3e-7 m); SMPLPP_SKIN = e | h | b | v puts every launch on that form.  The split-operand kernels address their basis images
// with 32-bit buffer offsets: a mesh whose image would reach 2 GiB (more than ~745k vertices for h, ~410k for b) takes the
// first form (64-bit addressing).  e keeps at most 4 skinning weights per vertex in registers and b at most 8: a model with
// more takes the next form.
inline std::pair<char, char> choose_forms(const char * env, int maxw, int64_t VGPn)
{
  const char e = env ? env[0] : 0;
  char forms[2] = {'e', 'h'};
  if(e == 'e' || e == 'h' || e == 'b' || e == 'v') forms[0] = forms[1] = e;
  for(char & f : forms)
  {
    if(f == 'h' && VGPn * HB_SLOTS * HB_IMG > 0x7fffff00LL) f = 'v';
    if(f == 'e' && VGPn * EB_KS * EB_IMG > 0x7fffff00LL) f = 'v';
    if(f == 'b' && VGPn * BB_KS * BB_B_BYTES > 0x7fffff00LL) f = 'v';
    if(f == 'e' && maxw > 4) f = 'b';
    if(f == 'b' && maxw > 8) f = 'v';
  }
  return {forms[0], forms[1]};
}
} // namespace smplpp_hip
