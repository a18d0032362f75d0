// Host-only plan of the assembled ILU(k) (gls_ilu_plan.cpp): everything gls_ilu_attach decides from the mesh and the
// constraints alone -- the system-matrix pattern, the distance-2 probe colouring, the renumbering, the ILU(fill)
// pattern, the multicolor node groups, the probe lists. Plain std::vector structs: no device, no context.
//
// Two calls, because across ranks a collective exchange on the device side sits between them:
//   ilu_plan_patterns  -> the patterns, the probe colours, the probe of each DoF
//   (complete owned rows: the caller's column-tag exchange turns the full pattern into remote records)
//   ilu_plan_finish    -> everything else
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace gls {

// the layout the multicolor solve kernels read (gls_launch.hpp's kMaxGroupRows / kGroupDesc; gls_ilu.cpp asserts
// that they agree)
constexpr int kPlanMaxGroupRows = 4;
constexpr int kPlanGroupDesc = 24;

struct IluPlanInput {
  int dim = 0, k = 0, kp = 0;
  int64_t n_vnodes = 0, n_pnodes = 0, n_cells = 0;
  std::vector<int32_t> cell_vnodes;  // [n_cells][(k+1)^dim]
  std::vector<int32_t> cell_pnodes;  // [n_cells][(kp+1)^dim]; empty: the pressure sits on the velocity nodes
  std::vector<int64_t> con_dofs;     // zero_constraints: Dirichlet DoFs and lines
  std::vector<int64_t> h_dof, h_off, h_master;  // the lines (hanging nodes, slip on curved walls); h_off empty: none
  // across ranks: owned velocity / pressure nodes come first, ghosts after; n_owned < 0: not distributed
  int64_t n_owned = -1, n_owned_p = -1;
  int fill = 0, ordering = 0;  // GLS_ILU_ORDER_CM / GLS_ILU_ORDER_MULTICOLOR
  int64_t block_dofs = 0;      // block-Jacobi subdomain size; 0: one block
};

struct IluCsr {  // rows of DoFs or nodes, each sorted
  std::vector<int64_t> off, col;
};

// a neighbour rank's contribution to an owned row (complete owned rows): in probe round `round`, send-list slot
// `slot` carries entry (i, j)
struct IluRemoteEntry {
  int32_t round, slot;
  int64_t i, j;
};

struct IluPlan {
  // ---- ilu_plan_patterns
  int64_t n = 0, n_nodes = 0;  // DoFs; unified nodes (velocity nodes, then separate pressure nodes)
  bool complete = false;       // distributed: complete owned rows
  std::vector<int64_t> dnode;  // DoF -> unified node
  std::vector<int32_t> dslot;  // DoF -> its slot in the node's probes (component; dim = pressure)
  std::vector<char> cons;      // constrained DoFs, the ghosts joined to them
  std::vector<char> fcons;     // ... before the ghosts join (the view of the complete rows)
  IluCsr a;                    // system-matrix rows in the context's numbering (owned block across ranks)
  IluCsr graph;                // node graph of a
  IluCsr fa;                   // complete rows: the full local pattern (the tag exchange reads it)
  std::vector<int> color;      // probe colour of each node
  int slots = 0;               // probes per colour: dim + 1
  int n_probe_colors = 0, n_probes = 0;
  int probe_of(int64_t d) const { return color[(size_t)dnode[(size_t)d]] * slots + dslot[(size_t)d]; }
  // ---- ilu_plan_finish
  int n_blocks = 1, n_order_colors = 0, n_rounds = 0;
  std::vector<int32_t> dcolor;  // multicolor: each DoF's colour
  std::vector<int32_t> perm;    // DoF -> its row in the renumbered matrix
  std::vector<int64_t> rowp, didx;  // the ILU(fill) pattern, each row's diagonal entry
  std::vector<int32_t> col;
  int64_t nnz_a = 0;  // entries of the system matrix (inside the blocks)
  // multicolor solves (mc_solve: no entry couples two nodes of one colour)
  bool mc_solve = false;
  std::vector<int32_t> grow, cg;   // node group -> first row; colour -> first node group
  std::vector<int64_t> lsp, usp;   // per row: L / U split entries
  std::vector<int64_t> desc;       // per node group: kPlanGroupDesc int64
  std::vector<uint8_t> mc_wl, mc_wu;  // per colour: wavefronts per node group in the lower / upper solve
  int64_t maxrow = 0;              // longest row
  std::vector<int64_t> moff;       // factorization position map: per row, its first entry (n + 1)
  // probes
  std::vector<int64_t> pdoff, peoff;   // per probe: offsets into pdofs and (pent, prow)
  std::vector<int32_t> pdofs, prow, pdpid, pepid;
  std::vector<int64_t> pent;
  std::vector<int64_t> ghost_diag;     // diagonal entries of the ghost (identity) rows
  // the neighbours' entries, per round
  std::vector<int64_t> ru, rr;
  std::vector<int32_t> ruoff, rslot;
};

// Both return 0, or -1 with the message in err.
int ilu_plan_patterns(const IluPlanInput &in, IluPlan &P, std::string &err);
int ilu_plan_finish(const IluPlanInput &in, const std::vector<IluRemoteEntry> &remote, int n_rounds, IluPlan &P,
                    std::string &err);

}  // namespace gls
