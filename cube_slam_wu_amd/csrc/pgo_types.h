// pgo_types.h -- what pgo_host.cpp hands to pgo_kernels.hip (pose-graph optimisation over Sim(3) vertices, include/cubeslam_hip.h: cs_pgo_*).
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

// The graph and one linearisation of it as the kernels see them.  Unknowns: the free vertices that have an edge, 7 each, in vertex order
// (vcol[v] = first column, -1 for a fixed or edge-less vertex); the damped system is the dense lower triangle S[r n + c] (ba_types.h).
struct PgoView {
  int nv, ne, n;                    // vertices, edges, unknowns
  double* est;                      // nv x 8 (Sim3::operator[] order)
  const unsigned char* fix_scale;   // nv
  const int* vcol;                  // nv
  const int *ei, *ej;               // ne
  const double* meas;               // ne x 8
  const double* info;               // ne x 49, row-major
  // per edge, written by pgo_edge_kernel
  double *err, *Ji, *Jj;            // ne x 7, ne x 49 (row-major 7 x 7: row = error component), ne x 49
  double *Hii, *Hij, *Hjj;          // ne x 49: J_i^T Omega J_i, J_i^T Omega J_j, J_j^T Omega J_j
  double *bi, *bj;                  // ne x 7: -J^T Omega e
  double* chi2_each;                // ne
  // vertex-major gather: the edges of vertex v are inc_edge[inc_ptr[v] .. inc_ptr[v + 1]), bit 0 of inc_side = the vertex is the edge's j
  const int *inc_ptr, *inc_edge;
  const unsigned char* inc_side;
  double *S, *b, *x, *diag;         // n x n, n (right-hand side kept), n (right-hand side in / solution out), n (H_jj without lambda)
  double* rec;                      // [0] chi2  [1] x^T (lambda x + b)  [2] max |H_jj|
};

enum { PGO_EDGES_PER_BLOCK = 2, PGO_REDUCE_T = 256 };

void pgo_launch_edges(const PgoView& v, hipStream_t st);                       // e, J, the products and chi2_each of every edge
void pgo_launch_errors(const PgoView& v, hipStream_t st);                      // err and chi2_each only (after a trial's update)
void pgo_launch_chi2(const PgoView& v, hipStream_t st);                        // rec[0] <- sum of chi2_each, a fixed tree
void pgo_launch_assemble(const PgoView& v, double lambda, hipStream_t st);     // S <- H + lambda I (the graph's blocks), b, x <- b, diag, rec[2]
void pgo_launch_scale(const PgoView& v, double lambda, hipStream_t st);        // rec[1] <- sum x (lambda x + b), a fixed tree
void pgo_launch_update(const PgoView& v, hipStream_t st);                      // est <- exp(x_v) est for every vertex with a column
void pgo_launch_se3(const double* est, int nv, double* Tcw7, hipStream_t st);  // [sR t] -> [R t / s], SE3Quat::toVector order
void pgo_launch_correct_points(const double* est_init, const double* est, int n, const int* ref, const double* xyz_in, double* xyz_out, hipStream_t st);

}  // namespace cs
