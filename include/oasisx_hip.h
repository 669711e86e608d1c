/*
 * oasisx_hip.h -- C ABI of the MI355X (gfx950) implementation of the per-time-step
 * IPCS hot path of oasisx's FractionalStep_AB_CN.
 *
 * The reference (ComputationalPhysiology/oasisx, pure Python) has no FFI of its
 * own: on this path it calls DOLFINx (assembly, set_bc) and PETSc (Mat/Vec/KSP).
 * Every entry point below replaces one such call site; the file:line cited is
 * the reference call it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (text via ox_last_error());
 *   - all pointers marked "device" are HIP device pointers owned by the caller
 *     (the Python host allocates them with torch); the library owns no field data;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     stream-ordered and only ox_ksp_solve blocks (it returns host-visible results);
 *   - all floating point data is float64, all indices int32, offsets int64;
 *   - multi-component vectors are interleaved: v[row*ncomp + comp];
 *   - process model: ONE process per GPU and one call at a time per HOST THREAD.  The library keeps
 *     per-thread scratch (the reduction scratch of ox_dot / ox_remove_mean, the pinned copy of the
 *     Krylov state of ox_ksp_solve, the Jacobi-diagonal hook of the merged CG epilogue): two solves in flight from
 *     ONE thread on different streams would share it; host threads that each drive their own handles (e.g. the ranks
 *     of a partitioned job rehearsed inside one process, tests/test_gpu_threads_rehearsal.py) do not.  The profiler's
 *     event list (ox_profile_*) is per process: profile from one thread.  The product runs one rank per process, the
 *     reference's model (one PETSc solve at a time per MPI rank);
 *   - an x handed to ox_spmv / ox_ksp_solve on a matrix with a pair-slot stream (ps_*) must be FINITE in
 *     every owned and ghost column: a slot multiplies two adjacent columns and its second half may be the
 *     code of 0.0 (0 * Inf = NaN where the entry streams would not touch that column; -0.0 sums can come
 *     out as +0.0).  With finite x the results are bit-identical to the entry streams.
 *
 * Matrix layout: SELL-64 ("sliced ELLPACK", one slice = the 64 rows one CDNA
 * wavefront owns, lane = row).  Inside slice s with width w_s (multiple of OX_KV)
 * entry k of lane l sits at
 *      slice_ptr[s] + (k / OX_KV) * 64 * OX_KV + l * OX_KV + (k % OX_KV)
 * so that a wave reads 64 * 16 B of values with one dwordx4 load per lane.
 * The dof numbering of a function space IS the SELL row order (rows are grouped
 * by length inside windows at setup), so no row permutation is applied.
 */
#ifndef OASISX_HIP_H
#define OASISX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OX_KV 2          /* entries of one row stored contiguously (16-B value loads) */
#define OX_ROW_BLOCK_WAVES 8              /* slices (= waves) per row block of the one-launch assembly kernels        */
#define OX_ROW_BLOCK_LDS (134 * 1024)     /* bytes of LDS accumulators per row block: 4 slices of 65-entry rows (the
                                             vertex rows of a P2 box mesh), rows of up to 268 entries               */
#define OX_SLICE 64      /* rows per slice = wavefront width */

/* KSPConvergedReason values the step functions return (reference ksp.py:78,
 * fracstep.py:681,684 assert > 0). */
#define OX_CONVERGED_RTOL 2
#define OX_CONVERGED_ATOL 3
#define OX_CONVERGED_ITS 4
#define OX_DIVERGED_ITS (-3)
#define OX_DIVERGED_DTOL (-4)
#define OX_DIVERGED_BREAKDOWN (-5)
#define OX_DIVERGED_NANORINF (-9)

#define OX_KSP_CG 1      /* PETSc "cg"   */
#define OX_KSP_BCGS 2    /* PETSc "bcgs" */
#define OX_KSP_CG_SINGLE 3 /* PETSc "cg" with -ksp_cg_single_reduction: Chronopoulos-Gear recurrences, ONE
                              merged reduction (one all-reduce in partitioned runs) per iteration */
#define OX_KSP_BCGS_MERGED 4 /* "bcgs" with merged reductions: TWO synchronisation points (all-reduces) per
                              iteration instead of three -- rhat.v behind the first mat-vec; t.t, t.s, rhat.s,
                              rhat.t, s.s behind the second give omega, rho and |r| together (|r| by the
                              recurrence |s - omega t|^2, as PETSc's pipelined / improved BiCGStab variants do).
                              Same Krylov space; iteration counts within +-2 of OX_KSP_BCGS.  Inside the loop the
                              convergence test reads the RECURRENCE norm sqrt(max(0, s.s - 2 omega t.s + omega^2 t.t)),
                              which near 1e-10..1e-12 relative can sit below the norm of the stored residual; once it
                              reports convergence the solver sums r.r of the STORED residual (one extra reduction per
                              solve), takes reason and result->rnorm from that -- the test PETSc's KSPBCGS makes
                              (reference ksp.py:76) -- and, where it fails, re-seeds the shadow residual and carries on */

#define OX_KSP_CG_MERGED 5 /* "cg", one right-hand side, ONE synchronisation point and THREE kernels per iteration instead of
                             two and five: the mat-vec q = A p also sums p.q and q.D^-1 q, from which alpha and -- with
                             r' = r - alpha q:  r'.z' = r.z - 2 alpha q.z + alpha^2 q.D^-1 q,  q.z = p.q - beta_old p.q_old (z =
                             D^-1 r = p - beta_old p_old, A symmetric), plain algebra without any orthogonality assumption --
                             beta follow together; one kernel then updates x, r and p and sums the TRUE r.z, |z|^2 and p.q_old
                             for the next point (the carried r.z is replaced every iteration: no drift; the convergence test
                             sees the true |D^-1 r|, one point later: one surplus mat-vec per solve).  Same Krylov space;
                             iteration counts equal to OX_KSP_CG's up to rounding.  With ncomp > 1 the call runs OX_KSP_CG */
#define OX_KSP_CG_MG 6 /* "cg" preconditioned by the V-cycle of an ox_mg hierarchy (ox_ksp_options.mg) instead of the Jacobi
                          diagonal: PETSc's KSPCG + PCGAMG; on a mesh-partitioned operator pc_type bjacobi + sub_pc_type gamg.
                          One right-hand side */

/* SELL-64 matrix: pattern + one value array (PETSc Mat on this path). */
typedef struct {
  int64_t n_rows;            /* rows owned by this rank                                  */
  int64_t n_cols;            /* local columns (owned + ghost)                            */
  int32_t n_slices;          /* ceil(n_rows / 64)                                        */
  int32_t n_dict;            /* entries of vdict (0: no value dictionary)                   */
  const int64_t *slice_ptr;  /* device [n_slices+1], entry offsets, multiples of 64*OX_KV */
  const int32_t *cols;       /* device [slice_ptr[n_slices]] (padding: own row, value 0) */
  double *vals;              /* device [slice_ptr[n_slices]]                             */
  /* optional 16-bit column stream (ox_sell_compress_cols); both NULL = int32 columns only */
  const uint16_t *cols16;    /* device [slice_ptr[n_slices]] codes: cols[e] =
                                cbase[e / (64*OX_KV)][code >> 15] + (code & 0x7fff)         */
  const int32_t *cbase;      /* device [slice_ptr[n_slices] / (64*OX_KV)][2]; [0] < 0 at the
                                first pair of a slice: that slice is read from cols         */
  /* optional value dictionary for matrices with <= 256 distinct values (mass / stiffness on
   * meshes of congruent cells): vals[e] == vdict[vcode[e]] bit for bit; used with cols16 */
  const uint8_t *vcode;      /* device [slice_ptr[n_slices]]                                */
  const double *vdict;       /* device [n_dict]                                             */
  /* optional, mesh-partitioned operators: the slices listed with the INTERIOR ones first (no ghost
   * column in any of their rows), then the boundary ones.  With it the distributed mat-vecs start
   * the halo exchange, multiply the interior slices while it is in flight, and finish with the
   * boundary slices (DOLFINx/PETSc do the same inside MatMult; reference fracstep.py:453,497,632). */
  const int32_t *ib_slices;  /* device [n_slices] or NULL                                   */
  int32_t n_interior;        /* leading entries of ib_slices that are interior              */
  int32_t n_wb_interior;     /* LDS-window stream of a mesh-partitioned operator: its window blocks are listed with the
                                INTERIOR ones (no ghost column in any row of any of their slices) first; this many.
                                The overlapped mat-vec multiplies blocks [0, n_wb_interior) while the halo exchange is in
                                flight and the others after it (0 with ib_slices set: no interior block)  */
  /* optional pair-slot stream of a value-dictionary matrix (ox_pair_stream_size / _fill; all NULL =
   * not built).  A slot multiplies TWO adjacent columns: y += vdict[a] * x[col] + vdict[b] * x[col+1],
   * one 16-byte gather instead of two 8-byte ones -- the SpMV on these matrices is bound by the number
   * of vector-memory instructions (16 cycles of the address unit each), not by bytes.
   * Slots keep the stored order of the row's entries (an entry whose successor is the next column
   * shares its slot; any other entry gets b = the code of 0.0), so sums are bit-identical. */
  const int64_t *ps_ptr;     /* device [n_slices+1], offsets into ps_code, multiples of 256;
                                bit 0 set by _fill: that slice is read from cols / vcode;
                                bits 1-3 set by _fill: slots of the slice's last group of 4 that
                                any row uses (the others are padding: no gather is issued)    */
  const uint32_t *ps_code;   /* device [ps_ptr[n_slices]]; slot j of lane l of slice s at
                                ps_ptr[s] + (j/4)*256 + l*4 + j%4: bits 0-14 column offset, bit 15
                                which base, bits 16-23 code a, bits 24-31 code b                */
  const int32_t *ps_base;    /* device [ps_ptr[n_slices] / 256][2] column bases per group of 4
                                slots x 64 lanes                                                */
  /* optional LDS-window stream (ox_window_size / ox_window_fill; all NULL / 0 = not built).  The mat-vecs on the
   * velocity matrices are bound by their gather instructions, not by bytes (every x operand of a lane = row kernel
   * is one gather wave-instruction: DESIGN.md 3).  A WINDOW BLOCK = up to 8 slices (512 rows) whose rows lie close
   * together in the mesh; the sorted list of the distinct columns its entries touch is its window.  The kernel
   * copies x[window] into LDS once (|window| gathers instead of one per entry: 6-9 x fewer) and reads every operand
   * from there through a 16-bit index.  Same entries, same per-row order of fused multiply-adds: bit-identical
   * results.  Blocks whose window exceeds the kernel's LDS budget are multiplied from `cols` as before. */
  const int32_t *wb_slices;  /* device [n_wblocks][8] slice ids of each block (-1: none)                */
  const uint16_t *wb_waves;  /* device [n_wblocks]: 2 bits per slot j = the wave (0..3) that multiplies
                                slice wb_slices[b][j] -- a schedule that balances the slices' widths     */
  const int64_t *wb_ptr;     /* device [n_wblocks+1] offsets into wlist                                  */
  const int32_t *wlist;      /* device [wb_ptr[n_wblocks]] ascending distinct columns of each block      */
  const int64_t *wt_ptr;     /* device [n_slices+1]: first TILE of each slice in wcode / wvcode; a tile = 2 storage
                                pairs (4 entries) of the 64 lanes, lane-contiguous: entry 2j + i (i = 0, 1) of pair
                                2t + j of lane l of slice s at ((wt_ptr[s] + t) * 64 + l) * 4 + 2j + i; a slice of
                                npair pairs has ceil(npair / 2) tiles, the surplus pair of an odd slice's last tile is
                                unused.  One 8-byte (wcode) and one 4-byte (wvcode) load per lane serve 4 entries     */
  const uint16_t *wcode;     /* device [wt_ptr[n_slices] * 256]: cols[e] == wlist[wb_ptr[b] + wcode[tile slot of e]]
                                for every slot e of a slice of block b                                    */
  const uint8_t *wvcode;     /* device [wt_ptr[n_slices] * 256] or NULL: vcode in the tile layout (per matrix, with
                                its value dictionary: ox_window_retile)                                    */
  int32_t n_wblocks;         /* 0: no window stream                                                      */
  int32_t w_max;             /* largest window (entries)                                                 */
  /* per-matrix schedule knobs of the mat-vec (results never depend on them: every storage level multiplies the same
   * entries in the same order).  0 = the library's defaults */
  int32_t levels;            /* storage levels ox_spmv may use on THIS matrix: OX_SPMV_LEVELS(mask) with mask bit 0
                                nontemporal matrix stream, 1 the 16-bit column stream, 2 the 1-byte value codes, 3 the
                                pair-slot stream, 4 the LDS-window stream -- each where the matrix carries it; 0 = all */
  int32_t w_cap;             /* LDS-window stream: window entries the launch holds in LDS (0 = 6144 / 3072 / 2176 for
                                1 / 2 / 3 right-hand sides); a block whose window is larger multiplies from `cols`  */
} ox_sell;
#define OX_SPMV_LEVELS(mask) (32 | ((mask) & 31))

/* Cells of the mesh as the element kernels read them. */
typedef struct {
  int32_t gdim;              /* 2 (triangles) or 3 (tetrahedra)                          */
  int32_t reserved;
  int64_t n_cells;
  const double *geom;        /* device [n_cells][gs]: grad(lambda_1..d) row-major, |detJ|;
                                gs = 6 (2-D, one pad) or 10 (3-D)                        */
} ox_cells;

/* dof -> cell adjacency of one row space in the same SELL-64 row order:
 * pair (t, lane) of slice s sits at adj_ptr[s] + t*64 + lane. */
typedef struct {
  int32_t n_slices;
  int32_t nd;                /* dofs per cell of the ROW space                           */
  const int64_t *adj_ptr;    /* device [n_slices+1]                                      */
  const int32_t *adj_cell;   /* device [pairs], -1 = padding                             */
  const uint8_t *adj_loc;    /* device [pairs], local index of the row dof in the cell   */
} ox_adj;

/* Halo plan + communicator for mesh-partitioned runs (NULL = single GPU). */
typedef struct ox_dist ox_dist;
/* Smoothed-aggregation AMG hierarchy (ox_mg_create, below) */
typedef struct ox_mg ox_mg;

typedef struct {
  int32_t reason[4];         /* per component, KSPConvergedReason                        */
  int32_t its[4];            /* per component, iterations taken                          */
  double rnorm[4];           /* per component, final preconditioned residual norm        */
  double bnorm[4];           /* per component, preconditioned norm of b                  */
  int32_t resumed[4];        /* OX_KSP_BCGS_MERGED: times the column was re-opened because its STORED residual failed
                                the test its recurrence norm had passed (0 for every other method)  */
} ox_ksp_result;

/* ---- set-up: mesh -> spaces -> patterns (ox_setup.hip) ----------------------------------
 * What DOLFINx does for the reference behind functionspace() / create_matrix() /
 * create_sparsity_pattern() (reference fracstep.py:187-216,293-300,315,324,336,352).  The objects
 * own their device arrays; the *_view calls hand out pointers that stay valid until the object is
 * destroyed (pointers named *_host are host memory).  A binding needs nothing but these calls and
 * numpy arrays of vertex coordinates and cell->vertex indices. */
typedef struct ox_mesh ox_mesh;
typedef struct ox_space ox_space;
typedef struct ox_rect ox_rect;

typedef struct {
  int32_t gdim, tile_bits;
  int64_t n_vertices, n_cells;
  double lo[3], span[3];     /* bounding box                                                */
  const double *coords;      /* device [n_vertices][gdim]                                   */
  const int32_t *cells;      /* device [n_cells][gdim+1], KERNEL order (tiled by centroid)  */
  const int32_t *cell_perm;  /* device [n_cells]: kernel cell index -> caller's cell index  */
  ox_cells cells_struct;     /* geometry of the cells in kernel order, as the kernels take it */
  int32_t lattice;           /* 1: vertices on a tensor grid (tiled lexicographic order), 0: Z-order curve;
                                with lo / span / tile_bits / n_cells: the frame ox_mesh_create_sub takes  */
  int32_t reserved;
} ox_mesh_info;

typedef struct {
  ox_sell sell;              /* the pattern (vals == NULL: copy the struct and set vals per matrix) */
  int64_t size, nnz;         /* storage slots (padding included) / real entries             */
  int64_t n_compressed;      /* slots read through the 16-bit column stream                 */
  const int32_t *row_len;    /* device [n_rows]                                             */
  int32_t n_bins;            /* width bins of the assembly launches (ox_assemble_matrix)    */
  const int64_t *bin_ptr_host;
  const int32_t *bin_width_host;
  const int32_t *bin_slices; /* device [n_slices]                                           */
  const int32_t *widths_host;/* host [n_slices]                                             */
  /* row blocks of the one-launch assembly (ox_assemble_first / ox_assemble_matrix, row_blocks = 1): block b owns the
   * CONSECUTIVE slices [row_blk_ptr[b], row_blk_ptr[b+1]) -- at most OX_ROW_BLOCK_WAVES of them, their storage slots
   * together at most OX_ROW_BLOCK_LDS / 8 (greedy, in storage order); row_blk_entries = the largest block's slots
   * (sizes the launch's LDS).  n_row_blocks = 0: a slice is wider than the budget, use the width bins. */
  int32_t n_row_blocks;
  int32_t reserved_rb;
  const int32_t *row_blk_ptr;/* device [n_row_blocks + 1]                                   */
  int64_t row_blk_entries;
} ox_pattern_info;

typedef struct {
  int32_t degree, nd, pw, gdim; /* dofs per cell; stride of the position bytes              */
  int64_t n_dofs, n_edges, n_pairs;
  const int32_t *cell_dofs;     /* device [n_cells][nd], kernel cell order, final numbering */
  const double *x;              /* device [n_dofs][gdim] dof coordinates                    */
  const int32_t *rank_initial;  /* device [n_dofs]: vertex id (or n_vertices + edge id) -> dof */
  const uint64_t *edge_keys;    /* device [n_edges]: min_vertex * n_vertices + max_vertex, ascending */
  ox_adj adj;                   /* dof -> cell adjacency in slice order                      */
  const uint8_t *adj_pos;       /* device [n_pairs][pw]                                      */
  const int64_t *pair_start;    /* device [n_dofs+1]: cells per dof = pair_start[r+1] - pair_start[r] */
  ox_pattern_info pattern;      /* square operator on the space (M, K, A share it: fracstep.py:293-294) */
  int64_t n_faces;              /* degree 3 on tetrahedra: faces (one dof each: initial id n_vertices + 2 n_edges + face) */
  const uint64_t *face_keys;    /* device [n_faces]: (v0 * n_vertices + v1) * n_vertices + v2 of the sorted triple, ascending */
} ox_space_info;

typedef struct {
  int32_t pw;
  const uint8_t *pos;           /* device [rows' n_pairs][pw]: in-row positions of the column space's cell dofs */
  ox_pattern_info pattern;
} ox_rect_info;

/* LDS-window stream of a space's square pattern: the arrays ox_sell.wb_* / wlist / wt_ptr / wcode point to */
typedef struct {
  int32_t n_wblocks, w_max;     /* window blocks (8 slices each); entries of the largest window           */
  int64_t n_list, n_tiles;      /* entries of wlist; tiles of wcode (256 codes each)                      */
  int64_t n_over_16bit;         /* slices in blocks whose window exceeds 65535 entries (codes 0: read from cols) */
  const int32_t *wb_slices;
  const uint16_t *wb_waves;
  const int64_t *wb_ptr;
  const int32_t *wlist;
  const int64_t *wt_ptr;
  const uint16_t *wcode;
} ox_window_info;

/* coords [n_vertices][gdim] f64, cells [n_cells][gdim+1] int32 (any order, any orientation);
 * on_device: the two pointers are device pointers; tile_bits < 0: default.
 * Cells (and later the dofs) are ordered for the kernels: a lattice mesh (few distinct values per
 * coordinate) by y-z tiles of whole x-lines, any other mesh along a Z-order curve. */
int ox_mesh_create(const double *coords, int64_t n_vertices, const int32_t *cells, int64_t n_cells, int gdim,
                   int on_device, int tile_bits, ox_mesh **out);
int ox_mesh_view(const ox_mesh *mesh, ox_mesh_info *view);
int ox_mesh_destroy(ox_mesh *mesh);
/* scalar Lagrange space of degree 1 or 2 (functionspace(mesh, ("Lagrange", k)), fracstep.py:187-216);
 * window: rows per length-sorting window of the SELL-64 numbering (< 64: the default 4096). */
int ox_space_create(const ox_mesh *mesh, int degree, int window, ox_space **out);
/* The same with a choice of the dof order: order_flags bit 0 = BRICK order on lattice meshes -- (tile, brick_z, brick_y,
 * brick_x, z, y, x) with bricks of about 8 points a side instead of whole x-lines: the rows of 8 consecutive slices
 * then share a compact window of columns, what the LDS-window SpMV (ox_sell.wb_*) needs.  The lane = row kernels
 * gather worse in this order (mass mat-vec 487 -> 630 us at 128^3): only together with the window stream. */
int ox_space_create_ordered(const ox_mesh *mesh, int degree, int window, int order_flags, ox_space **out);
/* One rank's piece of a mesh-partitioned space (what DOLFINx's functionspace() returns on a distributed mesh,
 * reference fracstep.py:186-216): built from that rank's cells only (its own cells + one ghost layer).
 *   ox_mesh_create_sub   the part as a mesh of its own (vertices renumbered 0..n-1 in ascending global id) whose
 *                        ordering keys use the WHOLE mesh's frame -- bounding box lo/span, lattice flag, tile bits,
 *                        cell count -- so every part orders its cells and dofs as the whole mesh would;
 *   ox_space_create_part owner: device [n_initial] owner rank of every initial dof of the part (its vertices, then
 *                        its edges by ascending vertex pair for degree 2).  Dofs owned by `rank` come first (tile
 *                        order, window-sorted by row length: the rows of every pattern of the space), the ghosts
 *                        behind them ordered by (owner, initial id) -- the order in which the owners send them.
 *                        pattern.sell.n_rows = owned dofs, n_cols = n_dofs = owned + ghosts.  n_dofs_whole: dofs of
 *                        the whole space (resolution of the ordering keys). */
int ox_mesh_create_sub(const double *coords, int64_t n_vertices, const int32_t *cells, int64_t n_cells, int gdim,
                       int on_device, const double *lo, const double *span, int lattice, int tile_bits,
                       int64_t n_cells_whole, ox_mesh **out);
int ox_space_create_part(const ox_mesh *mesh, int degree, int window, const int32_t *owner, int64_t n_initial, int rank,
                         int64_t n_dofs_whole, ox_space **out);
/* A mesh with PERIODIC boundaries: faces of its bounding box identified by axis-aligned translations (DESIGN.md,
 * "Periodic boundaries").  coords / cells are the geometric mesh as for ox_mesh_create: cell order, cell geometry and
 * everything that reads points (the cell locator, output) use them.  topo_cells [n_cells][gdim+1] int32 lists the same
 * cells over vertex CLASSES 0 .. n_topo_vertices - 1 (identified vertices share a class; every class must occur, every
 * id is range-checked): spaces created on the mesh take their edge keys, initial dof ids, pattern and adjacency from
 * it, so identified vertices and edges are ONE dof and every row is assembled completely by the row kernels.  The
 * caller guarantees that two distinct geometric edges of non-identified position never join the same two classes (at
 * least three cells across every periodic axis).
 *   hi_cut [3]     per axis: hi_k - tolerance on a periodic axis, +infinity (HUGE_VAL) on the others.  Dof
 *                  coordinates (ox_space_info.x) are written from the (cell, local node) pairs whose node lies below
 *                  hi_cut on every axis: x[:, k] is in [lo_k, hi_k) on periodic axes, and the midpoint of an edge that
 *                  crosses the seam lies at the seam, not in the middle of the domain.
 * On such a mesh ox_space_info.n_dofs is the reduced count, rank_initial / edge_keys are indexed by vertex class
 * (class id, or n_topo_vertices + edge id; keys min_class * n_topo_vertices + max_class).  Degree 1 and 2, one GPU:
 * ox_space_create with degree 3 and ox_space_create_part refuse the mesh; ox_space_create fails when some dof has no
 * image below hi_cut on every axis (hi_cut or topo_cells do not describe the mesh). */
int ox_mesh_create_periodic(const double *coords, int64_t n_vertices, const int32_t *cells, const int32_t *topo_cells,
                            int64_t n_topo_vertices, int64_t n_cells, int gdim, int on_device, int tile_bits,
                            const double *hi_cut, ox_mesh **out);
int ox_space_view(const ox_space *space, ox_space_info *view);
/* LDS-window stream of the space's square pattern (M, K, A share it), built on the first call and owned by the space:
 * copy the pointers into the ox_sell of every matrix on the pattern (the value codes of a dictionary matrix are
 * re-tiled per matrix: ox_window_retile).  Worth it where the rows of 8 consecutive slices share their columns:
 * any mesh in Z-order, box meshes in brick order (ox_space_create_ordered). */
int ox_space_windows(ox_space *space, ox_window_info *view);
/* The same with blocks whose window holds more than split_entries columns cut in two (4 + 4 slices; 0 = never,
 * ox_space_windows): for patterns whose mat-vecs run with three right-hand sides -- the LDS budget of such a launch is
 * 2176 window entries, a block beyond it multiplies from the int32 columns.  One-column launches (budget 6144) lose
 * ~9 % to the extra lists: the velocity pattern yes, the pressure pattern no.  A call with another split_entries than
 * the stream was built with builds it anew (views handed out before are stale then). */
int ox_space_windows_split(ox_space *space, int split_entries, ox_window_info *view);
int ox_space_destroy(ox_space *space);
/* pattern of a mixed operator, rows = dofs of `rows`, columns = dofs of `cols` (fracstep.py:315,336,352) */
int ox_rect_create(const ox_space *rows, const ox_space *cols, ox_rect **out);
int ox_rect_view(const ox_rect *rect, ox_rect_info *view);
int ox_rect_destroy(ox_rect *rect);
/* Value dictionary of a matrix that will not change any more (M, K, Ap, the rectangular operators):
 * vals [n_slots][ncomp] device doubles.  At most 256 distinct bit patterns: dict (device, room for 256,
 * ascending as signed 64-bit integers), *n_dict of them, and codes (device; ncomp == 1: one byte per
 * slot, ncomp 2..3: one uint32 per slot, byte c = code of component c).  More: *n_dict = 0. */
int ox_value_dictionary(const double *vals, int64_t n_slots, int ncomp, void *codes, double *dict, int *n_dict,
                        void *stream);
/* Pair-slot stream of a matrix that carries a value dictionary (A->vcode, A->vdict, ncomp == 1) whose
 * dictionary contains 0.0.  row_len: device [n_rows] entries per row (ox_pattern_info.row_len).
 * _size writes ps_ptr (device [n_slices+1]) and returns the number of uint32 codes in *n_codes (0: not
 * available for this matrix); _fill writes ps_code [n_codes] and ps_base [n_codes/256][2], marks in
 * ps_ptr (bit 0) the slices whose columns do not fit two 15-bit windows per group -- they keep their
 * int32 columns -- and returns their number in *n_wide.  Then set A->ps_ptr / ps_code / ps_base. */
int ox_pair_stream_size(const ox_sell *A, const int32_t *row_len, int64_t *ps_ptr, int64_t *n_codes, void *stream);
/* Re-tile a per-slot array of A's pattern (elem_bytes = 1: vcode, 2: 16-bit codes) from the pair layout of
 * slice_ptr into the tile layout of wt_ptr (ox_sell.wt_ptr); unused entries of a slice's last tile are zeroed. */
int ox_window_retile(const ox_sell *A, const int64_t *wt_ptr, const void *src, int elem_bytes, void *dst, void *stream);
int ox_pair_stream_fill(const ox_sell *A, const int32_t *row_len, int64_t *ps_ptr, uint32_t *ps_code,
                        int32_t *ps_base, int64_t *n_wide, void *stream);
/* Unfolded copy of a field on a periodic mesh, for output: dst [n_images][ncomp] = src [n_src][ncomp] read through
 * image_dof [n_images] (the dof of every geometric image of a node: the points a writer lists); an index outside
 * [0, n_src) gives NaN.  All device pointers. */
int ox_gather_images(const double *src, int64_t n_src, const int32_t *image_dof, int64_t n_images, int ncomp, double *dst,
                     void *stream);
/* plain device memory for callers without a device array library (numpy + ctypes) */
int ox_malloc(size_t bytes, void **out);
int ox_free(void *p);
int ox_memset(void *p, int value, size_t bytes, void *stream);
int ox_synchronize(void *stream);

/* ---- library -------------------------------------------------------------------- */
int ox_version(void);
const char *ox_last_error(void);
int ox_sell_kv(void);
/* device of the current context: compute units and name (diagnostics for bench.py) */
int ox_device_info(int *n_cu, char *name, int name_len);

/* ---- S1/S2: Mat.mult (reference fracstep.py:452,501,541,615,638,642) -------------- */
/* y[row*ncomp+c] = sum_k A[row,k] * x[col_k*ncomp+c]; ncomp in 1..3. */
int ox_spmv(const ox_sell *A, const double *x, double *y, int ncomp, const ox_dist *dist,
            void *stream);

/* Set-up: 16-bit column stream of a pattern for ox_spmv / ox_ksp_solve (10 instead of 12 bytes
 * per stored entry; results are bit-identical).  cols16: [slice_ptr[n_slices]] uint16, cbase:
 * [slice_ptr[n_slices] / (64*OX_KV)][2] int32, both caller-allocated device arrays that the caller then
 * sets in ox_sell.  n_compressed (host, may be NULL): stored entries now read as 16 bit. */
int ox_sell_compress_cols(const ox_sell *A, uint16_t *cols16, int32_t *cbase, int64_t *n_compressed,
                          void *stream);

/* ---- S2: Mat.mult of the pre-assembled rectangular operators (low_memory_version = False,
 *      reference fracstep.py:499-502, 540-542, 642).  One SELL pattern, gdim values per entry
 *      (A->vals holds [slot][gdim]).
 *      v2s = 0: y[row][d] = base[row][d] + scale * sum_k vals[k][d] * x[col_k]     (P_i ps, G_i dp)
 *      v2s = 1: y[row]    = base[row]    + scale * sum_k sum_d vals[k][d] * x[col_k][d]  (sum_i D_i u_i)
 *      base may be NULL. */
int ox_spmv_multi(int v2s, int gdim, const ox_sell *A, const double *x, const double *base, double scale,
                  double *y, const ox_dist *dist, void *stream);
/* A9: one-off assemble_matrix of those operators (fracstep.py:392-404) into zero-initialised
 * [slot][gdim] values.  family 0: p*v.dx(i)*dx (rows V, cols Q); 1: p.dx(i)*v*dx (rows V, cols Q);
 * 2: u.dx(i)*q*dx (rows Q, cols V).  adj/adj_pos: adjacency of the ROW space with the in-row
 * positions of the COLUMN space's cell dofs. */
int ox_assemble_rect(int family, int row_degree, int col_degree, const ox_cells *cells, const ox_adj *adj,
                     const uint8_t *adj_pos, int pw, const ox_sell *A, void *stream);

/* ---- V1: Vec axpy/copy/scale on .x.array (fracstep.py:432-434,456-458,506,604,622,690-693) */
/* z = a*x + b*y elementwise over n doubles (x, y, z may alias). */
int ox_axpby(int64_t n, double a, const double *x, double b, const double *y, double *z,
             void *stream);
/* V1: out[c] = sum_i x[i*ncomp+c]*y[i*ncomp+c] (Vec.norm/dot, fracstep.py:524); host result. */
int ox_dot(int64_t n_rows, int ncomp, const double *x, const double *y, double *out_host,
           const ox_dist *dist, void *stream);

/* ---- V2: set_bc(vec,[bc]) (reference bcs.py:135-139, fracstep.py:518,550) ---------- */
/* b[dofs[k]*ncomp+comp] = g[k]. */
int ox_set_bc(double *b, const int32_t *dofs, const double *g, int64_t n, int ncomp, int comp,
              void *stream);

/* A11: adding the assembled outlet term to the RHS (reference fracstep.py:461-465):
 * b[rows[k]*ncomp+comp] += scale * y[k]; rows must be unique (no atomics). */
int ox_scatter_add(double *b, const int32_t *rows, const double *y, int64_t n, int ncomp, int comp,
                   double scale, void *stream);

/* ---- S4: Mat.zeroRowsLocal(rows, diag) (fracstep.py:471-472); keeps columns -------- */
int ox_zero_rows(const ox_sell *A, const int32_t *rows, int64_t n, double diag, void *stream);
/* The same, and au[row][c] = diag * u1[row][c] for the zeroed rows (au may be NULL): the identity rows of the
 * product A u1 that ox_assemble_first (args.a_u1) hands to the tentative-velocity solve (fracstep.py:470-472 + :521). */
int ox_zero_rows_au(const ox_sell *A, const int32_t *rows, int64_t n, double diag, double *au,
                    const double *u1, int ncomp, void *stream);
/* DOLFINx assemble_matrix(..., bcs) on the pressure Laplacian (fracstep.py:379):
 * rows AND columns flagged in is_bc[] -> identity. */
int ox_zero_rows_cols(const ox_sell *A, const uint8_t *is_bc, double diag, void *stream);

/* ---- A1/A2/A3: one-off assemble_matrix of mass / stiffness (fracstep.py:373-380) ---- */
/* kind 0: u*v*dx, kind 1: inner(grad u, grad v)*dx on the square Lagrange space `space` over `cells`.  Overwrites A->vals.
 * `space` is the view ox_space_view filled (or a caller's own struct); the row-assembly entry points read ONLY
 *   degree, pw, cell_dofs ([n_cells][nd]), adj, adj_pos ([pairs][pw]: per (row, cell) pair the in-row index k of every
 *   cell dof), pattern.{n_bins, bin_ptr_host, bin_slices, bin_width_host, n_row_blocks, row_blk_ptr, row_blk_entries}.
 * row_blocks = 0: one launch per width bin -- bin b covers bin_slices[bin_ptr_host[b] .. bin_ptr_host[b+1]) (device
 *   list) whose rows are at most bin_width_host[b] entries wide (sizes the per-wave LDS accumulator).
 * row_blocks = 1: ONE launch over the slices in storage order (round 5): row block b = the consecutive slices
 *   [row_blk_ptr[b], row_blk_ptr[b+1]), one per wave of a 512-thread block, accumulators for row_blk_entries storage
 *   slots per block.  An error on a pattern with n_row_blocks == 0: the caller chooses the form.  The width bins send
 *   the slices of one length-sort window -- one compact region of the mesh -- to up to ten launches, each of which
 *   fetches that region's cell records and coefficients again (refined Delaunay mesh: 95.9 GB of HBM traffic per call
 *   for ~22 GB of streams); in storage order the rows of a cell meet in one L2.  Per slice the same operations in the
 *   same order: bit-identical results. */
int ox_assemble_matrix(int kind, const ox_cells *cells, const ox_space_info *space, const ox_sell *A, int row_blocks,
                       void *stream);
/* w[row] = int phi_row dx (body-force vector for constant f: fracstep.py:387-390, and
 * the weights of assemble_scalar(phi*dx): fracstep.py:585-590). */
int ox_assemble_weights(int degree, const ox_cells *cells, const ox_adj *adj, int64_t n_rows,
                        double *w, void *stream);
/* Load vector of a non-constant source: b[row] = int f phi_row dx, the `force * v * dx` of a body force that is a
 * UFL expression (fracstep.py:284-289, assembled once at :387-390) and the `inner(function, v) * dx` of a
 * Projector (function.py:75,110-113).  The caller tabulates: fq[cell][q] = f at the n_q quadrature points of every
 * cell (kernel cell order), wphi[q][i] = w_q phi_i(x_q) on the reference simplex (any rule, any of the n_d basis
 * functions of the space `adj` belongs to); the kernel forms, per row, sum over its (cell, i) pairs in adjacency
 * order of |det J_cell| * sum_q wphi[q][i] fq[cell][q] -- one lane per row, no atomics, fixed order. */
int ox_assemble_load_vector(const ox_cells *cells, const ox_adj *adj, int64_t n_rows, int n_d, int n_q,
                            const double *wphi, const double *fq, double *b, void *stream);

/* ---- A4 + S3 + S1, fused: assemble_first (fracstep.py:432-469) ---------------------- */
/* With uab = 1.5*u1 - 0.5*u2 already formed (ox_axpby), for every row:
 *   C   = assemble_matrix(inner(dot(uab, nabla_grad(u)), v)*dx)            (:435-437)
 *   Ar  = -0.5*C + (1/dt)*M - 0.5*nu*K                                     (:438-442)
 *   b_first[:, i] = Ar @ u1[:, i] + b0[:, i]                               (:449-458)
 *   A   = -Ar + (2/dt)*M                                                   (:468-469)
 * M, K, A share one SELL pattern (fracstep.py:293-294).  space, row_blocks: as for ox_assemble_matrix.
 * a_u1 (device [n_rows][gdim]) = (the assembled A) @ u1 row by row, with the entry order and operations of ox_spmv:
 * where u1 is also the initial guess of the tentative-velocity solve (fracstep.py:521 with
 * -ksp_initial_guess_nonzero) it is that solve's first mat-vec (ox_ksp_options.ax0), once the rows ox_zero_rows_au
 * turns into identity rows have been set to u1.
 * nut (device [n_cells], kernel cell order: ox_cell_viscosity): C is replaced by
 * C + sum_e nut[e] K_e (K_e: the stiffness matrix of cell e), i.e. A = M/dt + C/2 + (nu K + K_nut)/2 and b_first to
 * match: the Laplacian form div(nut grad u) of a viscosity that varies per cell.  Same launch forms, same epilogue;
 * nut = 0 everywhere gives the bits of nut == NULL. */
typedef struct {
  const double *uab, *u1, *b0;  /* device, interleaved [n][gdim]                                          */
  double *b_first;
  double dt, nu;
  double *a_u1;                 /* optional: (assembled A) @ u1, NULL = not formed                         */
  const double *nut;            /* optional: per-cell viscosity, kernel cell order; NULL = the
                                   constant-viscosity instantiations (not "nut = 0")                       */
} ox_first_args;
int ox_assemble_first(const ox_cells *cells, const ox_space_info *space, const ox_sell *A, const ox_sell *M,
                      const ox_sell *K, const ox_first_args *args, int row_blocks, void *stream);

/* ---- a viscosity per cell for ox_first_args.nut: eddy-viscosity models and generalised-Newtonian laws ---- */
/* nut[e], e in kernel cell order (the order of cells->geom and cell_dofs), from g = grad uab at the cell's centroid:
 * S = sym(g), gd = sqrt(2 S:S), Delta = |cell|^(1/gdim).  uab interleaved [n_u][gdim], cell_dofs [n_cells][nd] of the
 * velocity component space of `degree` (1, 2, 3).  One launch, one lane per cell.
 *   model 0, Smagorinsky: nut = C Delta^2 gd with
 *     C = coefficient^2, or
 *     C = (coefficient D)^2 with `damping` (van Driest): D = 1 - exp(-y+ / a_plus),
 *       y+ = dist[e] u_tau / nu.  dist[e], nearest[e] (device, kernel cell order): the wall distance of the cell's centroid
 *       and the position of its nearest wall facet (ox_walldist_query); u_tau = sqrt(|wss[nearest[e]]|) with wss (device
 *       [n_facets][gdim]) the kinematic wall shear of those facets (ox_wall_stress), or the constant u_tau where wss is
 *       NULL.  nearest[e] outside [0, n_facets) writes NaN and reads nothing; wss = 0 gives D = 0 and nut = 0.  Or
 *     C = cs2[k cs2_stride] with `cs2` (device; the dynamic model): k = cell_bin[e] (cell_bin given;
 *       k < 0: C = 0; k >= n_coef: NaN) or k = e (cell_bin NULL, n_coef = n_cells).
 *   model 1, WALE (gdim = 3 only): (coefficient Delta)^2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4)), 0 where the
 *     denominator is 0; Sd = sym(g g) - tr(g g)/3 I.
 *   models 2-4, the generalised-Newtonian laws: nut = max(nu(gd) - base, 0); the caller runs the
 *     step at nu = base.  params: HOST array of n_params doubles (5, 4, 4), finite.
 *     2, Carreau-Yasuda, params = {nu0, nu_inf, lam, n, a}: nu = nu_inf + (nu0 - nu_inf) (1 + (lam gd)^a)^((n - 1)/a),
 *        base = min(nu0, nu_inf);  3, Cross, params = {nu0, nu_inf, lam, m}: nu = nu_inf + (nu0 - nu_inf) / (1 + (lam gd)^m),
 *        same base;  4, power law, params = {k, n, nu_min, nu_max}: nu = min(max(k gd^(n - 1), nu_min), nu_max),
 *        base = nu_min; at gd == 0: nu_max for n < 1, nu_min for n > 1, the clipped k for n == 1.
 * A field the chosen form does not read must be NULL or 0, or the call is refused (on the host, nothing is written):
 * coefficient with cs2 or a law, params with models 0 and 1, damping or cs2 with models 1-4, damping together with cs2 (not
 * instantiated), cs2_stride / n_coef / cell_bin without cs2. */
typedef struct {
  const double *dist;      /* [n_cells]                                       */
  const int32_t *nearest;  /* [n_cells]                                       */
  const double *wss;       /* [n_facets][gdim] or NULL                        */
  double u_tau;            /* used where wss is NULL; finite, >= 0            */
  double nu, a_plus;       /* > 0                                             */
  int64_t n_facets;
} ox_vandriest;
typedef struct {
  int model, degree;            /* 0 Smagorinsky, 1 WALE, 2 Carreau-Yasuda, 3 Cross, 4 power law                    */
  const int32_t *cell_dofs;     /* device [n_cells][nd]                                                            */
  const double *uab;            /* device, interleaved [n_u][gdim]                                                 */
  double *nut;                  /* device [n_cells]                                                                */
  double coefficient;           /* models 0, 1 (Cs, Cw) where cs2 is NULL; >= 0, squared on the host               */
  const double *params; int n_params;  /* models 2-4: HOST array                                                   */
  const ox_vandriest *damping;  /* model 0, optional (host struct of device tables)                                */
  const double *cs2;            /* model 0, optional: device table of coefficients                                 */
  int64_t cs2_stride, n_coef;   /* >= 1; 1 .. INT32_MAX                                                            */
  const int32_t *cell_bin;      /* device [n_cells] or NULL                                                        */
} ox_viscosity_args;
int ox_cell_viscosity(const ox_cells *cells, const ox_viscosity_args *args, void *stream);
/* ---- the dynamic Smagorinsky model: the Germano-Lilly procedure ----
 * NS = gdim (gdim + 1) / 2.  All arrays are device arrays in kernel cell order / vertex-class order; every launch has one
 * summation order and no atomics, so equal inputs give equal bits.  Counts must fit int32 (indices are int32).
 * The test filter of a per-cell q: q_v = sum_{c in patch(v)} |c| q_c / sum |c| (the cells of a vertex in ascending order),
 * q^_c = the mean of q_v over the cell's gdim + 1 vertices.  ptr [n_vertices + 1], idx [ptr[n_vertices]]: the vertex ->
 * cell CSR; cell_verts [n_cells][gdim + 1]: the vertex classes of a cell.  An index out of range writes NaN and reads
 * nothing.
 *   ox_dynamic_cells:    rec[c][gdim + NS + 2] = {u at the centroid, upper triangle of S = sym(grad uab) row by row,
 *                        D s, |c|}, D = |c|^(2/gdim), s = sqrt(2 S:S); cell_dofs, uab as for ox_cell_viscosity
 *   ox_dynamic_vertices: mom[v][gdim + 3 NS] = {u, u u^T, S, D s S} filtered to the vertex (upper triangles)
 *   ox_dynamic_products: lm[c][2] = {Ld:M, M:M}, L = (u u^T)^ - u^ u^^T, Ld = L - tr L / gdim I,
 *                        M = filter_ratio^2 D |S^| S^ - (D s S)^, |S^| = sqrt(2 S^:S^); filter_ratio > 1
 *   ox_dynamic_bin_sums: partials[chunk][2] = sum over the chunk's cells of vol[c vol_stride] {lm[c][0], lm[c][1]}; order,
 *                        chunks, n_chunks: the plan of ox_profile_cells
 *   ox_dynamic_bin_coefficients: bins[b][4] = {sum LM, sum MM, -(1/2) LM / MM, that clipped to [0, cs2_max]}; the clipped
 *                        value is 0 where sum MM is not positive; a NaN stays a NaN.  One wave per bin.
 *   ox_patch_filter_vertices / ox_patch_filter_cells: the two halves of the filter for q [n_cells][k], k = 1 or 2;
 *                        n_idx = ptr[n_vertices]
 *   ox_dynamic_clip:     cs2[i] = the clipped -(1/2) pairs[i][0] / pairs[i][1], as above
 * nut then comes from ox_cell_viscosity with cs2 = the clipped coefficients, per cell or per bin. */
int ox_dynamic_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab, double *rec,
                     void *stream);
int ox_dynamic_vertices(int gdim, int64_t n_vertices, const int32_t *ptr, const int32_t *idx, int64_t n_cells,
                        const double *rec, double *mom, void *stream);
int ox_dynamic_products(int gdim, int64_t n_cells, const int32_t *cell_verts, int64_t n_vertices, const double *rec,
                        const double *mom, double filter_ratio, double *lm, void *stream);
int ox_dynamic_bin_sums(int64_t n_cells, const double *lm, const double *vol, int64_t vol_stride, const int32_t *order,
                        const int32_t *chunks, int64_t n_chunks, double *partials, void *stream);
int ox_dynamic_bin_coefficients(int64_t n_bins, const int32_t *bin_chunk_ptr, const double *partials, double cs2_max,
                                double *bins, void *stream);
int ox_patch_filter_vertices(int k, int64_t n_vertices, const int32_t *ptr, const int32_t *idx, int64_t n_cells,
                             int64_t n_idx, const double *q, const double *vol, int64_t vol_stride, double *qv,
                             void *stream);
int ox_patch_filter_cells(int k, int gdim, int64_t n_cells, const int32_t *cell_verts, int64_t n_vertices, const double *qv,
                          double *qf, void *stream);
int ox_dynamic_clip(int64_t n, const double *pairs, double cs2_max, double *cs2, void *stream);
/* ---- the full stress form of a per-cell viscosity ---- */
/* The transposed term of div(nut (grad u + grad u^T)), explicit in uab, added to b in place:
 * b[r][i] += scale * sum_e nut[e] int_e sum_j d(uab)_j/dx_i d(phi_r)/dx_j, rows r < n_rows of the velocity component space
 * of `degree` (1, 2, 3; adj and cell_dofs of that space), b and uab interleaved [n][gdim], nut [n_cells] in kernel cell
 * order.  lane = row, fixed summation order, no atomics: two launches on equal inputs give equal bits. */
int ox_assemble_stress_transpose(int degree, const ox_cells *cells, const int32_t *cell_dofs, const ox_adj *adj,
                                 int64_t n_rows, const double *uab, const double *nut, double scale, double *b,
                                 void *stream);

/* ---- flow diagnostics and running statistics: read-only on the solver's fields ---- */
/* Per cell e (kernel cell order, one lane per cell) of the velocity u (interleaved [n_u][gdim], cell_dofs [n_cells][nd] of
 * the component space of `degree` 1, 2, 3), with g = grad u, S = sym g, W = skew g:
 *   cell_integrals[e][7] (optional) = {|cell|, 1/2 int |u|^2, int 2 S:S, (nu + nut[e]) int 2 S:S, 1/2 int |curl u|^2,
 *                                      int (div u)^2, int div u}, exact for the element (nut optional: NULL = nu alone);
 *   fields[e][NF] (optional), NF = 4 + (gdim == 2 ? 1 : 3), values at the cell's centroid:
 *                                     {dt max_a |u . grad lambda_a|, sqrt(2 S:S), tr g, 1/2 (W:W - S:S), curl u (1 | 3)};
 *   partials[(n_cells + 255) / 256][8] = per 256-cell block the seven sums and the maximum of the first field, which is
 *                                     NaN if any of its operands is.  Fixed reduction tree, no atomics. */
int ox_flow_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *u, const double *nut, double dt,
                  double nu, double *fields, double *cell_integrals, double *partials, void *stream);
/* ring[slot][0..7] (ring: device [capacity][8]) = the seven sums and the (NaN-propagating) maximum over the n_blocks rows
 * of partials.  One block, fixed order. */
int ox_flow_reduce(int64_t n_blocks, const double *partials, double *ring, int64_t capacity, int64_t slot, void *stream);
/* West's weighted incremental update per dof i < n of x (device, row i at x + i ldx, ncomp = 1, 2, 3 values):
 *   W' = W_old + w, delta = x - mean, mean += (w / W') delta, cov[i][k] += (w W_old / W') delta_r delta_c for r <= c,
 *   k over the upper triangle row by row (00, 01, 02, 11, 12, 22); mean [n][ncomp], cov [n][ncomp (ncomp + 1) / 2].
 * W_old == 0: mean = x, cov = 0 (whatever they held).  w > 0.  One thread per dof, no atomics. */
int ox_stats_accumulate(int ncomp, int64_t n, const double *x, int64_t ldx, double w, double W_old, double *mean,
                        double *cov, void *stream);
/* Slab-averaged statistics.  The joint vector q has nq components (1, or gdim .. gdim + 2): the
 * first nc0 = (nq == 1 ? 1 : gdim) lie side by side in source 0 (row i at src[0] + i ld[0]), every further one is the
 * first value of row i of its own source; n_src = 1 + nq - nc0 <= 3 (src, ld: HOST arrays), all on cell_dofs [n_cells][nd]
 * of `degree`.  order (device int32): the sampled cells sorted by bin; chunks (device int32 [n_chunks][4], 16-byte
 * aligned) = {first entry of order, cells (<= 256), bin, 1 if those cells are consecutive}, no chunk crossing a bin.
 * One block per chunk, one lane per cell; with delta_i = q_i - shift[bin] (shift: device [n_bins][nq] or NULL = 0)
 *   partials[c] = [sum |cell|, s1 (nq), s2 (nq (nq + 1) / 2)],  s1[k] = sum int delta[k],  s2[k][l] = sum int delta[k]
 *   delta[l] for k <= l row by row, exact for the element.  Fixed reduction tree, no atomics. */
int ox_profile_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, int nq, int n_src,
                     const double *const *src, const int64_t *ld, const int32_t *order, const int32_t *chunks,
                     int64_t n_chunks, const double *shift, double *partials, void *stream);
/* One wave per bin b: V, S1, S2 = the sum of the partial rows bin_chunk_ptr[b] .. bin_chunk_ptr[b + 1] (fixed order), then
 * with d = S1 / V, g = shift[b] + d, a = w / (W_old + w):  mean[b] += a (g - mean[b]),  m2[b] += w (S2 / V - d d^T) +
 * W_old a (g - mean[b]) (g - mean[b])^T (upper triangle),  vol[b] = V.  shift may be mean itself.  seed != 0: mean[b] = d
 * and vol[b] = V alone (w, W_old and m2 unused).  sums (optional): [n_bins][1 + nq + nq (nq + 1) / 2] = V, S1, S2. */
int ox_profile_update(int nq, int64_t n_bins, const int32_t *bin_chunk_ptr, const double *partials, const double *shift,
                      double w, double W_old, int seed, double *mean, double *m2, double *vol, double *sums, void *stream);

/* ---- A6 / A8: assemble_vector(p * v.dx(i) * dx) and (dp.dx(i) * v * dx), all i at once
 *      (fracstep.py:487-497 and :618).  kind 0: out[r][i] = base[r][i] + scale * int p d_i(phi_r)
 *      kind 1: out[r][i] = base[r][i] + scale * int d_i(p) phi_r.  base may be NULL (=0). */
int ox_assemble_grad_vector(int kind, int row_degree, int p_degree, const ox_cells *cells,
                            const int32_t *cell_pdofs, const ox_adj *adj, int64_t n_rows,
                            const double *p, const double *base, double scale, double *out,
                            void *stream);
/* ---- A7: assemble_vector(div(u) * q * dx) scaled (fracstep.py:538,546):
 *      out[r] = scale * int div(u) psi_r,  u interleaved [n_u][gdim]. */
int ox_assemble_div_vector(int row_degree, int u_degree, const ox_cells *cells,
                           const int32_t *cell_udofs, const ox_adj *adj, int64_t n_rows,
                           const double *u, double scale, double *out, void *stream);

/* ---- Jacobi preconditioner setup: dinv[row] = 1 / A[row,row] (PCJACOBI) ------------- */
int ox_jacobi_setup(const ox_sell *A, double *dinv, void *stream);

/* ---- K1/K2/K3: KSP.solve (reference ksp.py:71-78; fracstep.py:521,578,634) ---------- */
/* ONE call solves A x = b with the Krylov method `ksp_type` (OX_KSP_*) on `ncomp` (1..3) right-hand sides that share A
 * (the velocity components share one matrix, fracstep.py:274,521), run in lockstep with per-component scalars; b and x
 * are interleaved [n][ncomp].  Left preconditioning by the Jacobi diagonal `dinv` (ox_jacobi_setup), or, with
 * OX_KSP_CG_MG, by one V-cycle z = B r of the hierarchy `opt->mg` (one right-hand side; dinv may be NULL and
 * opt->dinv_code is ignored; A is the operator of the hierarchy's level 0).  PETSc conventions: zero initial guess unless
 * opt->nonzero_guess, convergence on the preconditioned norm |B r| <= max(rtol |B b|, atol).  Scalars stay on the device;
 * the host reads the state every `check_every` iterations, and once all columns but one have finished the rest of the
 * solve runs on one-column vectors.  Every argument is checked before the first device call.
 *   work         ox_ksp_work_bytes_for(A, ncomp, ksp_type) bytes of device memory
 *   dist         NULL on one GPU.  Otherwise A (n_owned x n_local) is the partitioned operator: every mat-vec refreshes
 *                the ghosts of its operand (one halo exchange), dot products run over the owned rows and every
 *                synchronisation point all-reduces.  x's ghosts are NOT refreshed at the end (ox_halo_forward).  A
 *                timed-out peer fails the solve (ox_dist_status).
 * The options, in one block -- PETSc's KSP options (reference ksp.py:38-53 forwards any key to KSPSetFromOptions) and
 * this library's schedule knobs, per call instead of per process:
 *   divtol       -ksp_divtol: |B r| >= divtol |B b| ends the column with OX_DIVERGED_DTOL (KSPConvergedDefault; PETSc's
 *                default 1e4 -- "divergence=10000." in -ksp_view)
 *   max_restarts BiCGStab only.  0 = PETSc's KSPBCGS: a rho = rhat.r = 0 (or omega = 0) breakdown ends the solve with
 *                OX_DIVERGED_BREAKDOWN.  > 0: re-seed the shadow residual (rhat <- r) and continue, at most that many
 *                times per component (used when a direct solver was asked for)
 *   fold_blocks  one-column CG on one GPU: blocks of the folded update kernels; 0 = separate synchronisation points
 *                (five kernels per iteration), -1 = ox_ksp_default_fold_blocks()
 *   run_ahead    one-column solves queue one batch ahead of the state the host reads: 1 / 0, -1 = default (1)
 *   ax0          A x0 supplied by the caller (nonzero_guess only; NULL = computed here), device [n_rows][ncomp], the
 *                product with the x passed in: the velocity update has M u* at hand from its right-hand side
 *                (fracstep.py:615,634), so the solver's first mat-vec is skipped.  Same iterates
 *   dinv_code    a value dictionary of dinv (device [n_rows] bytes, dinv[i] == dinv_dict[dinv_code[i]] bit for bit,
 *                1 <= n_dinv_dict <= 256; ox_value_dictionary builds it where dinv takes <= 256 distinct values, as the
 *                diagonals of M and Ap do on meshes of congruent cells): the CG update kernels then read one byte per row
 *                instead of eight.  Same iterates
 *   mg           OX_KSP_CG_MG: the hierarchy; with dist != NULL that of the rank's owned-by-owned block (n_owned rows,
 *                ghost columns dropped), applied without communication, and NULL on a rank that owns no rows (it still
 *                takes part in every exchange and all-reduce)
 * ox_ksp_options_default fills in PETSc's defaults (rtol 1e-5, atol 1e-50, divtol 1e4, max_it 10000, zero guess) and
 * leaves ax0, dinv_code and mg NULL. */
typedef struct {
  double rtol, atol, divtol;
  int32_t max_it, nonzero_guess, check_every, max_restarts;
  int32_t fold_blocks, run_ahead;
  const double *ax0;
  const uint8_t *dinv_code;
  const double *dinv_dict;
  int32_t n_dinv_dict;
  int32_t reserved;
  const ox_mg *mg;
} ox_ksp_options;
int ox_ksp_options_default(ox_ksp_options *opt);
int ox_ksp_solve(int ksp_type, const ox_sell *A, const double *dinv, const double *b, double *x, int ncomp,
                 const ox_ksp_options *opt, void *work, size_t work_bytes, ox_ksp_result *result,
                 const ox_dist *dist, void *stream);
size_t ox_ksp_work_bytes(int64_t n_rows, int64_t n_cols, int ncomp, int ksp_type);
/* Workspace of a solve on THIS operator: ox_ksp_work_bytes sizes the partial-sum arrays for the lane = row grid; an
 * operator that carries an LDS-window stream may launch more blocks than that (one per window block).  Callers with the
 * ox_sell at hand use this one; ox_ksp_solve checks against it. */
size_t ox_ksp_work_bytes_for(const ox_sell *A, int ncomp, int ksp_type);

/* ---- Projector into a discontinuous P1 space (reference function.py:13-143 with the "DG" 1 target of its
 *      test_projector.py:26-35).  Dof (cell e, vertex a, component c) at (e * (gdim+1) + a) * ncomp + c, cells in
 *      the order of `cells`.  The mass matrix is block diagonal: its inverse is applied cell by cell in closed
 *      form (the reference asks PETSc for preonly + LU).
 *      ox_dg1_grad_rhs: b = assemble_vector(inner(grad(u), v) * dx), u a Lagrange P1 / P2 field (function.py:74-77,
 *      :110-119), ncomp = gdim;  ox_dg1_mass: out = M^-1 in (inverse != 0: KSP.solve, function.py:132) or M in. */
int ox_dg1_grad_rhs(int u_degree, const ox_cells *cells, const int32_t *cell_dofs, const double *u, double *b,
                    void *stream);
int ox_dg1_mass(int inverse, const ox_cells *cells, int ncomp, const double *in, double *out, void *stream);

/* ---- V3 + A10: nullspace.remove and mean shift (fracstep.py:573-574, 579-591) -------- */
/* m = (sum_{i<n} w[i]*x[i], all ranks) / wsum;  x[i] -= m for i < n_apply (owned + ghost rows);
 * w == NULL -> plain sum (arithmetic mean when wsum = global n). */
int ox_remove_mean(int64_t n, int64_t n_apply, double *x, const double *w, double wsum,
                   const ox_dist *dist, void *stream);

/* ---- measurement: per-kernel HIP-event timing on the launching stream (bench.py) ------- */
/* tags: 10*ncomp+epi for SpMV (epi 0 plain, 1 CG p.q, 2/3 BiCGStab), 100 assemble_first,
 * 110/111 grad vectors, 120 div vector. */
/* One-column CG on one GPU folds the iteration's synchronisation points into its update kernels (3 kernels per iteration
 * instead of 5; replaces nothing in the reference: its PETSc KSPCG has the same two reductions, ksp.py:71-78).  The number of
 * 1024-thread blocks those kernels run is a per-solve option (ox_ksp_options.fold_blocks); this is the library's default
 * for it: one block per compute unit.  Partitioned operators never fold (their points carry an all-reduce). */
int ox_ksp_default_fold_blocks(void);
/* Kernels one iteration of the given method launches on this operator with these options (reporting: bench.py);
 * partitioned != 0: the operator has a halo plan.  OX_KSP_CG_MG: -1 (the count is ox_mg_kernels_per_cycle(mg) + 6: the
 * mat-vec, two synchronisation points, three vector kernels). */
int ox_ksp_kernels_per_iteration(int ksp_type, const ox_sell *A, int ncomp, int check_every, int fold_blocks,
                                 int partitioned);
int ox_profile_begin(int max_records, int sample_every); /* time every sample_every-th launch per tag */
int ox_profile_end(void);
int ox_profile_get(int tag, long long key, long long *count, double *total_ms); /* key: the matrix's
                                   n_rows for SpMV records (tells the pressure matrix from the
                                   velocity matrix), -1 = any */

/* roctx ranges on the calling host thread (rocprofv3 --kernel-trace --marker-trace segments the trace by them):
 * FractionalStep_AB_CN brackets its six phase methods (fracstep.py:411-658) with them -- what PETSc's log stages are
 * to the reference.  No-ops without librocprofiler-sdk-roctx / libroctx64 or without a profiler attached. */
int ox_range_push(const char *name);
int ox_range_pop(void);

/* ---- Smoothed-aggregation AMG (PETSc's pc_type gamg) for one-column CG, OX_KSP_CG_MG (ox_amg.hip) --------------------
 * The hierarchy is built on the host (oasisx_amd/amg.py); the library keeps copies of the level descriptions below and
 * its own level vectors.  Level 0 is the caller's operator with all its storage levels; levels 1.. are plain-f64 SELL-64.
 * Level l < n_levels - 1 is smoothed by `degree` Chebyshev-Jacobi steps,  r = D^-1 (b - A x);  d = c_d d + c_r r;
 * x += d  with (c_d, c_r) = cheb[2 j], cheb[2 j + 1] (step 1: c_d = 0), the same polynomial before and after the coarse
 * correction, which goes through P (n_l x n_{l+1}) and R = P^T (n_{l+1} x n_l).  The coarsest level (A, P, R, cheb
 * unused) is solved with the dense row-major inverse `coarse_inv` (device [n_c * n_c]): a symmetric V-cycle. */
#define OX_MG_MAX_DEGREE 8
#define OX_MG_MAX_LEVELS 16
typedef struct {
  ox_sell A;             /* level operator                                   */
  ox_sell P;             /* prolongation to this level from the next coarser */
  ox_sell R;             /* restriction, R = P^T                             */
  const double *dinv;    /* device [n_rows]: 1 / diag(A)                     */
  int64_t n_rows;
  int32_t degree;        /* Chebyshev steps (mg_levels_ksp_max_it)           */
  int32_t reserved;
  double cheb[2 * OX_MG_MAX_DEGREE];
} ox_mg_level;
/* tail_rows: the levels of at most this many rows (and the coarse solve) run in ONE single-workgroup launch; <= 0: the
 * library's default */
int ox_mg_create(int n_levels, const ox_mg_level *levels, const double *coarse_inv, int tail_rows, ox_mg **out);
int ox_mg_destroy(ox_mg *mg);
/* z = B r: one V-cycle (device vectors of the fine level's rows) */
int ox_mg_apply(const ox_mg *mg, const double *r, double *z, void *stream);
/* kernel launches of one V-cycle (reporting) */
int ox_mg_kernels_per_cycle(const ox_mg *mg);

/* ---- Projected initial guesses (PETSc's -ksp_guess_type fischer) for repeated CG solves on one operator (ox_guess.hip)
 * Per column of an interleaved (n_rows x ncomp) block the object keeps k <= size A-orthonormal directions x~_j (model 1
 * also A x~_j; model 2 only x~_j) in device memory it owns.  n_rows: local rows (owned + ghost), n_owned: the operator's
 * rows; dot products run over the owned rows and are all-reduced on a partitioned operator (dist != NULL).  Nothing is
 * read back by the host: every call is stream-ordered on `stream`.
 *   ox_guess_form:   k = 0: nothing (*ax0_out = NULL).  Otherwise x <- x_w + sum_j x~_j (x~_j . (b - A x_w)) on all
 *                    local rows, x_w = x if nonzero_guess else 0; A x_w is ax_w (device [n_owned][ncomp]) or, when NULL,
 *                    one mat-vec.  Model 1: *ax0_out = A x (device, owned by the object) for ox_ksp_options.ax0.
 *   ox_guess_update: after a converged solve whose initial guess ox_guess_form formed (x's ghosts refreshed): adds the
 *                    A-orthonormalised d = x - x0 (d = x when k was 0); with k = size the basis restarts from x alone.
 *                    A direction with d.A d <= 1e-20 of its value before the orthogonalisation (or either <= 0) is kept as
 *                    a zero slot. */
typedef struct ox_guess ox_guess;
int ox_guess_create(int64_t n_rows, int64_t n_owned, int ncomp, int model, int size, ox_guess **out);
int ox_guess_destroy(ox_guess *g);
int ox_guess_reset(ox_guess *g);        /* k = 0 (the operator's values or layout changed) */
int ox_guess_dim(const ox_guess *g);    /* the current k */
size_t ox_guess_bytes(const ox_guess *g); /* device bytes of the basis (reporting) */
int ox_guess_form(ox_guess *g, const ox_sell *A, const double *b, double *x, int nonzero_guess, const double *ax_w,
                  const double **ax0_out, const ox_dist *dist, void *stream);
int ox_guess_update(ox_guess *g, const ox_sell *A, const double *x, const ox_dist *dist, void *stream);

/* ---- Point evaluation: cell locator, evaluation at points, probes (ox_probe.hip) ------------------------------------
 * Locator over the straight simplices of a mesh (coords [n_vertices][gdim], cells [n_cells][gdim + 1] int64, both on the
 * device), or over the cells cell_ids[n_ids] only (device, ASCENDING mesh cell ids; NULL: all cells): a uniform
 * background grid, about one cell per bin, per bin the ascending list of the cells whose bounding box -- grown by the
 * barycentric tolerance `tol` and the absolute `padding` -- overlaps it.  The object owns its device memory; creation
 * synchronises `stream`, the queries are stream-ordered and read nothing back.
 *   ox_locator_find: per point x[i][gdim] the LOWEST mesh cell id whose barycentric coordinates all are >= -tol (tol <=
 *                    the tolerance of the creation) into cells[i] (-1: none; points outside the grid's box touch no
 *                    memory) and those gdim + 1 coordinates into bary[i][gdim + 1] (NaN when none).
 *   ox_locator_bary: the barycentric coordinates of x[i] in the GIVEN mesh cell cells[i] (NaN for -1 or a cell that is
 *                    not in the locator). */
typedef struct ox_locator ox_locator;
int ox_locator_create(int gdim, const double *coords, int64_t n_vertices, const int64_t *cells, int64_t n_cells,
                      const int64_t *cell_ids, int64_t n_ids, double tol, double padding, void *stream, ox_locator **out);
int ox_locator_destroy(ox_locator *loc);
int ox_locator_info(const ox_locator *loc, int64_t *n_cells, int64_t *n_bins, int64_t *n_list, int *bins_per_axis3);
int ox_locator_find(const ox_locator *loc, int64_t n_points, const double *x, double tol, int64_t *cells, double *bary,
                    void *stream);
int ox_locator_bary(const ox_locator *loc, int64_t n_points, const double *x, const int64_t *cells, double *bary,
                    void *stream);
/* Values of a Lagrange field of degree 1..3 (P1, P2, the gll_warped P3 element; node order of the assembly kernels) at
 * located points.  cell_dofs [n_cells][nd]: the space's table in kernel cell order; field: interleaved block [n_rows][nc];
 * col = -1: all nc columns, else that one.  Point i -- the caller passes the points SORTED by cell_pos, so that the lanes
 * of a wave read neighbouring rows -- lies in the cell at kernel position cell_pos[i] (-1: none -> NaN) with barycentric
 * coordinates bary[i][gdim + 1]; its values go to out[perm[i] * ld + off + v] (perm == NULL: i), one lane per point, sums
 * in dof order.  ox_probe_sample writes the same into slot `slot` of a ring [capacity][n_points][ld] on `stream`. */
int ox_eval_points(int degree, int gdim, const int32_t *cell_dofs, int64_t n_cells, int64_t n_rows, int64_t n_points,
                   const int64_t *cell_pos, const double *bary, const int64_t *perm, const double *field, int nc, int col,
                   double *out, int64_t ld, int64_t off, void *stream);
int ox_probe_sample(int degree, int gdim, const int32_t *cell_dofs, int64_t n_cells, int64_t n_rows, int64_t n_points,
                    const int64_t *cell_pos, const double *bary, const int64_t *perm, const double *field, int nc, int col,
                    double *ring, int64_t capacity, int64_t slot, int64_t ld, int64_t off, void *stream);
/* Lagrangian tracers: every live particle (status 0) moves from t to t + dt through the velocity
 * v(x, theta) = fma(theta, u_b(x) - u_a(x), u_a(x)), theta in [0, 1] across the step, in `substeps` substeps of h = dt /
 * substeps by explicit Euler, the midpoint rule or classical RK4 -- one kernel, one lane per particle, nothing read back.
 * Substep s starts at theta_s = s / substeps; a stage at the local fraction c evaluates at theta = (s + c) / substeps.
 * Location: the substep's start lies in cell[i]; every later stage point and the end point take cell[i] again when
 * use_hint is set and all barycentric coordinates there are >= 0, else the LOWEST containing cell of the locator
 * (lambda >= -tol, as ox_locator_find).  A substep one of whose points lies in no cell leaves the particle at that
 * substep's start with status 1, t_exit = t + theta_s dt, cell -1; a non-finite velocity or an index out of range does the
 * same with status 2.  A completed substep adds h to age and |x_new - x_old| to path.
 *   loc: a whole-mesh locator (created with cell_ids == NULL) of the same gdim; n_mesh_cells == its cell count.
 *   cell_dofs [n_cells][nd]: the scalar space's table in kernel cell order (as ox_eval_points); cell_inv [n_mesh_cells]:
 *   mesh cell id -> kernel cell position; u_a, u_b: interleaved blocks [n_rows][nc], nc >= gdim, at theta = 0 and 1 (the
 *   same pointer twice: a steady field).  x [n][gdim], cell, status, age, path, t_exit [n]: the particles, read and
 *   written.  Arguments are checked on the host before the first device call; n == 0 launches nothing. */
#define OX_TRACER_EULER 0
#define OX_TRACER_RK2 1
#define OX_TRACER_RK4 2
#define OX_TRACER_MAX_SUBSTEPS 1024
typedef struct ox_tracer_args {
  const ox_locator *loc;
  int degree, gdim, nc;
  const int32_t *cell_dofs;
  int64_t n_cells, n_rows;
  const int64_t *cell_inv;
  int64_t n_mesh_cells;
  const double *u_a, *u_b;
  double t, dt;
  int substeps, scheme, use_hint;
  double tol;
  int64_t n;
  double *x;
  int64_t *cell;
  int32_t *status;
  double *age, *path, *t_exit;
} ox_tracer_args;
int ox_tracer_advance(const ox_tracer_args *args, void *stream);

/* Lagrangian averaging of the dynamic Smagorinsky model (Meneveau, Lund & Cabot 1996): one lane per
 * vertex class, float64, one launch.  With s_LM = -2 src[v][0], s_MM = 4 src[v][1] (src: the k = 2 vertex pass of
 * ox_patch_filter_vertices on {Ld:M, M:M}):
 *   first != 0:  F_MM = s_MM, F_LM = max(cs2_initial s_MM, cs2_floor s_MM), status 0, nothing is traced.
 *   first == 0:  x' = x[v] - h u[v u_stride ..], folded into [lo, hi) on every axis with periodic[k] != 0; its cell is
 *     hint[v] (a mesh cell id) when all barycentric coordinates there are >= 0, else the LOWEST containing cell of the
 *     locator (lambda >= -tol): the rule of ox_tracer_advance.  B = the P1 interpolant of f_old at x' through
 *     cell_verts[cell_inv[cell]], summed in local vertex order.  status 1 (no cell holds x'): B = f_old[v].
 *     T = time_scale delta[v] (F_LM F_MM)^(-1/8) of f_old[v], eps = (h/T) / (1 + h/T), 0 where the product is not positive
 *     and finite, NaN where it is NaN.  F_MM = eps s_MM + (1 - eps) B_MM, F_LM = max(eps s_LM + (1 - eps) B_LM,
 *     cs2_floor F_MM); a NaN passes the max.  status 2 (x' not finite, or hint / cell_inv / cell_verts out of range):
 *     both fields NaN, nothing read out of range.
 *   cs2v[v] = F_LM / F_MM clipped to [0, cs2_max], 0 where F_MM is not positive, NaN where either is NaN.
 * f_old, f_new [n_vertices][2] = {F_LM, F_MM} must differ (lanes read their neighbours' old values); cell_verts
 * [n_cells][gdim + 1] in kernel cell order, cell_inv [n_mesh_cells] as for ox_tracer_advance; loc: a whole-mesh locator.
 * Arguments are checked on the host before the first device call; n_vertices == 0 launches nothing. */
typedef struct ox_lagrangian_args {
  const ox_locator *loc;
  int gdim, first;
  int64_t n_vertices;
  const double *x;           /* [n_vertices][gdim]                              */
  const double *u;           /* row v: u + v u_stride, gdim entries             */
  int64_t u_stride;
  const int64_t *hint;       /* [n_vertices]                                    */
  const int64_t *cell_inv;   /* [n_mesh_cells]                                  */
  int64_t n_mesh_cells;
  const int32_t *cell_verts; /* [n_cells][gdim + 1]                             */
  int64_t n_cells;
  const double *src;         /* [n_vertices][2]                                 */
  const double *delta;       /* [n_vertices]                                    */
  const double *f_old;
  double *f_new;
  double *cs2v;              /* [n_vertices]                                    */
  int32_t *status;           /* [n_vertices]                                    */
  double h, time_scale, cs2_floor, cs2_max, cs2_initial, tol;
  int periodic[3];
  double lo[3], hi[3], period[3];
} ox_lagrangian_args;
int ox_dynamic_lagrangian(const ox_lagrangian_args *args, void *stream);

/* ---- Distance to the nearest wall facet (ox_probe.hip) ------------------------------------------
 * facet_xyz (device [n_facets][gdim][gdim]): the vertices of the wall facets, segments in 2-D and triangles in 3-D;
 * n_facets >= 1.  The object copies them, lays the locator's uniform grid over their bounding box (an axis without
 * extent gets one bin) and keeps per bin the ascending list of the facets whose box overlaps it.  bins3 (host int[3],
 * 1..1024 each, or NULL): the bins per axis instead of the computed ones; (1, 1, 1) is a brute-force search by the same
 * kernel.  Creation synchronises `stream`; queries are stream-ordered and read nothing back.
 *   ox_walldist_query: one lane per point x[i][gdim] (+ shift[gdim], host, NULL = 0): rings of bins of growing Chebyshev
 *       radius around the point's (clamped) bin until nothing outside them can be nearer; points outside the grid are
 *       legal.  dist[i] = the distance to the closest point of the nearest facet, nearest[i] = its position in
 *       facet_xyz; of facets at the same distance (bit for bit) the LOWEST position.  Both are the same bits whatever
 *       the grid.  A non-finite point: dist = NaN, nearest = -1.  merge != 0: (dist, nearest) hold an earlier result; it
 *       is kept where it is not larger (equal distance: the lower position) -- how periodic images are searched. */
typedef struct ox_walldist ox_walldist;
int ox_walldist_create(int gdim, const double *facet_xyz, int64_t n_facets, const int *bins3, void *stream,
                       ox_walldist **out);
int ox_walldist_destroy(ox_walldist *wd);
int ox_walldist_info(const ox_walldist *wd, int64_t *n_facets, int64_t *n_bins, int64_t *n_list, int *bins_per_axis3);
int ox_walldist_query(const ox_walldist *wd, int64_t n_points, const double *x, const double *shift, int merge,
                      double *dist, int32_t *nearest, void *stream);

/* ---- Inertial particles (ox_probe.hip) ----------------------------------------------------------
 * Point particles, one-way coupled: dx/dt = v, dv/dt = (f / tau_p)(u(x, t) - v) + beta g, with the tracers' field
 * u(x, theta) = fma(theta, u_b - u_a, u_a), beta = 1 - rho_f / rho_p, f = 1 (OX_PARTICLE_STOKES) or 1 + 0.15 Re_p^0.687,
 * Re_p = diam |u - v| / nu (OX_PARTICLE_SCHILLER_NAUMANN).  One lane per live particle (status 0), all substeps in
 * registers.  A substep of h = dt / substeps from (x, v) at theta_s = s / substeps: u0 = the field at x (in cell[i]); f of
 * (u0, v), frozen; tau_e = tau_p / f; w = u0 + tau_e beta g; tau_e == 0: E = phi = 0, else E = exp(-h / tau_e),
 * phi = tau_e (-expm1(-h / tau_e));  x_new = x + h w + phi (v - w), v_new = w + E (v - w)  (OX_PARTICLE_EXP1).
 * OX_PARTICLE_EXP2: the position of the same formulas with h / 2 is folded and located, u_m = the field there at
 * theta = (s + 1/2) / substeps, and the update uses w_m = u_m + tau_e beta g (f, tau_e of the start).
 * Every predictor and end point is folded into [lo, hi) on the axes with periodic[k] != 0 before it is located (the rule of
 * ox_tracer_advance); wraps[i][gdim] counts the images, so that x + wraps * period is the unfolded position; path adds
 * the unfolded step.  A point in no cell leaves the particle at the substep's start with status 1, t_exit = t + theta_s dt,
 * cell -1; a non-finite position or velocity or an index out of range does the same with status 2.  A second launch on the
 * same stream takes the particles that left in THIS call (every other lane returns at once): the nearest facet of
 * `walls` to the folded point that lay in no cell, by the ring walk of ox_walldist_query (ties: the lower position), goes
 * to facet[i]; where facet_action[facet] == 1 the status becomes 3 (deposited) and v = 0.
 *   loc, cell_dofs, cell_inv, u_a, u_b, x, cell, status, age, path, t_exit: as ox_tracer_args.  walls: a structure over the
 *   exterior facets, n_facets == its facet count == the length of facet_action.  v [n][gdim], wraps [n][gdim], facet [n]
 *   (-1: none), tau_p, diam, beta [n]: the particles; xq [n][gdim]: work space (the points that left).  nu >= 0 (> 0 for
 *   Schiller-Naumann).  Arguments are checked on the host before the first device call; n == 0 launches nothing. */
#define OX_PARTICLE_EXP1 0
#define OX_PARTICLE_EXP2 1
#define OX_PARTICLE_STOKES 0
#define OX_PARTICLE_SCHILLER_NAUMANN 1
typedef struct ox_particle_args {
  const ox_locator *loc;
  const ox_walldist *walls;
  int degree, gdim, nc;
  const int32_t *cell_dofs;
  int64_t n_cells, n_rows;
  const int64_t *cell_inv;
  int64_t n_mesh_cells;
  const double *u_a, *u_b;
  double t, dt;
  int substeps, scheme, drag, use_hint;
  double tol, nu;
  double g[3];
  int periodic[3];
  double lo[3], hi[3], period[3];
  const int32_t *facet_action; /* [n_facets] 1: deposit */
  int64_t n_facets;
  int64_t n;
  double *x, *v;
  int64_t *cell;
  int32_t *status;
  double *age, *path, *t_exit;
  int32_t *wraps, *facet;
  double *xq;
  const double *tau_p, *diam, *beta;
} ox_particle_args;
int ox_particle_advance(const ox_particle_args *args, void *stream);

/* ---- Passive scalar transport (ox_scalar.hip) ------------------------------------------------------------------------
 * The Crank-Nicolson system of a group of 1..OX_MAXC scalars (same diffusivity kappa, same Dirichlet rows) from the
 * matrices of the velocity step, in ONE pass over the shared SELL-64 pattern -- no element loop:
 *   A   : the velocity matrix as ox_assemble_first leaves it, M/dt + C(u_ab)/2 + nu K/2, BEFORE ox_zero_rows* on it
 *   A_c = A + s K                           (s = (kappa - nu)/2; written to Ac->vals, padding slots stay 0)
 *   b   = (2/dt) M c1 - A_c c1 + b0         (= (M/dt - C/2 - kappa K/2) c1 + b0; rows < n_rows)
 *   a_c1 = A_c c1                            (optional, may be NULL: bit-identical to ox_spmv(Ac, c1), the solver's ax0)
 * A, M, K, Ac share one pattern (equal slice_ptr); Ac has a value array of its own.  M and K are read through their
 * 1-byte value codes where BOTH carry a dictionary, as f64 otherwise.  c1, b0, b, a_c1: interleaved (n, ncomp) device
 * blocks.  The group's Dirichlet rows follow with ox_zero_rows_au(Ac, rows, n, 1.0, a_c1, c1, ncomp).  No atomics,
 * fixed order of sums: two runs give the same bits. */
int ox_scalar_rows(const ox_sell *A, const ox_sell *M, const ox_sell *K, const ox_sell *Ac, double s, double dt, int ncomp,
                   const double *c1, const double *b0, double *b, double *a_c1, void *stream);
/* The same system on a solver with a per-cell viscosity nut (ox_first_args.nut; ox_assemble.hip):
 * there A = M/dt + C/2 + nu K/2 + K_t/2 with K_t = sum_c nut[c] K_c, which is stored nowhere.  ONE launch set in the shapes
 * of ox_assemble_first (row_blocks as there) forms the rows of K_t once more in LDS -- the stiffness contraction alone, no
 * u_ab gathers, no convection turns -- and streams the slices as ox_scalar_rows does:
 *   A_c = A + s K + t K_t     per entry v = fma(t, kt, fma(s, k, a));   s = (kappa - nu)/2,  t = (1/Sc_t - 1)/2
 *   b, a_c1 as for ox_scalar_rows (a_c1 bit-identical to ox_spmv(Ac, c1)).
 * nut: device [n_cells] in kernel cell order, read-only (the array the last ox_assemble_first read).  cells / space: those
 * of ox_assemble_first.  nut == 0 everywhere gives the bits of ox_scalar_rows.  No atomics to global memory, fixed order. */
int ox_scalar_rows_cellvisc(const ox_cells *cells, const ox_space_info *space, const ox_sell *A, const ox_sell *M,
                            const ox_sell *K, const ox_sell *Ac, const double *nut, double s, double t, double dt,
                            int ncomp, const double *c1, const double *b0, double *b, double *a_c1, int row_blocks,
                            void *stream);
/* SUPG stabilisation of a scalar group (streamline-upwind Petrov-Galerkin).  Per cell c, with
 * G[a] = grad lambda_a and k = degree:
 *   w_c   = u_ab at the centroid                                     (the frozen advecting velocity of the stabilising terms)
 *   tau_c = scale ([time_term] (2/dt)^2 + (k q_c)^2 + (2 k^2 kappa_c g_c)^2)^(-1/2),   q_c = sum_a |w_c . G[a]|,
 *           g_c = sum_a |G[a]|^2,   kappa_c = kappa + inv_sct nut[c]  (nut == NULL: kappa)
 * ox_supg_cells: one lane per cell; rec: device [(gdim + 1) n_cells], a structure of arrays in kernel cell order,
 * rec[d n_cells + c] = w_c[d], rec[gdim n_cells + c] = tau_c.  w_c = 0 gives a finite tau_c; a w_c that is not finite
 * gives tau_c = NaN.  cell_dofs, uab: those of ox_cell_viscosity. */
int ox_supg_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab, const double *nut,
                  double kappa, double inv_sct, double dt, double scale, int time_term, double *rec, void *stream);
/* ox_scalar_rows_supg: the sibling of ox_scalar_rows_cellvisc (same launches, same LDS accumulators, row_blocks as there):
 *   N_ij = sum_c tau_c int_c (w_c . grad phi_i) phi_j,   S_ij = sum_c tau_c int_c (w_c . grad phi_i)(w_c . grad phi_j)
 *   A_c  = A + s K + t K_t + N/dt + S/2      per entry v = fma(t, acc, fma(s, k, a)), acc = the rows of K_t + (N/dt + S/2)/t from LDS
 *   b    = (2/dt) M c1 - A_c c1 + b0 + N ((2/dt) c1 + fh)          (the last term per lane in registers, from the cells' dofs)
 *   a_c1 = A_c c1                             (optional; bit-identical to ox_spmv(Ac, c1))
 * rec: what ox_supg_cells wrote.  nut may be NULL (no model, or t = 0): then t is not read (t = 1 in the lines above).  fh: the nodal interpolant of
 * the source, an interleaved (n, ncomp) block as c1.  The second-derivative term tau (w . grad phi_i) kappa lap c is
 * dropped (zero for P1).  w = 0 everywhere gives the bits of ox_scalar_rows_cellvisc with the same nut and t (the accumulator
 * rows are formed by the sibling's operations), and with nut == NULL those of ox_scalar_rows.  No atomics to global
 * memory, fixed order of sums, no scratch. */
int ox_scalar_rows_supg(const ox_cells *cells, const ox_space_info *space, const ox_sell *A, const ox_sell *M,
                        const ox_sell *K, const ox_sell *Ac, const double *nut, const double *rec, double s, double t,
                        double dt, int ncomp, const double *c1, const double *b0, const double *fh, double *b, double *a_c1,
                        int row_blocks, void *stream);

/* ---- Scalars that drive the flow, scalar fluxes through walls (ox_scalar.hip) ------------------
 * Boussinesq force of 1..OX_MAXC coupled scalars onto the interleaved (n, gdim) block b (b_first of the velocity step), in
 * ONE pass over the mass matrix M.  Term t reads column col of the interleaved (n, nc) blocks c1, c2 (terms may come from
 * different groups: nc and col are per term; c2 == NULL: no second level):
 *   d_t[j] = (c1[j nc + col] + 0.5 (c1[j nc + col] - c2[j nc + col])) - ref          (c2 == NULL: c1[j nc + col] - ref)
 *   y_t[r] = sum_e M[r,e] d_t[col_e]     stored entry order, from 0, one fused multiply-add per entry (ox_spmv's operations)
 *   b[r gdim + i] += sum_t coef[t][i] y_t[r], terms ascending, rows < n_rows.
 * A component i whose coefficients are all zero is neither read nor written.  M is read through its 1-byte value codes
 * where it carries a dictionary, as f64 otherwise.  `terms` is a HOST array (copied into the kernel arguments).  No
 * atomics, a fixed order: two runs give the same bits. */
typedef struct {
  const double *c1, *c2;
  int32_t nc, col;
  double ref;
  double coef[3];
} ox_buoy_term;
int ox_buoyancy_rows(const ox_sell *M, int gdim, int n_terms, const ox_buoy_term *terms, double *b, void *stream);
/* Diffusive flux of column col of the interleaved (n, nc) block c through exterior facets; facets and records as for
 * ox_wall_stress (sorted by tag; a record outside the tables leaves NaN).  With the outward unit normal n, the measure
 * |f| and the exact facet means gbar of grad c and cbar of c (compile-time facet means of the P1 / P2 / P3 basis):
 *   q[i] = -kappa n . gbar   (a positive q leaves the domain),   fq[i] = |f| q[i],   cbar[i];   device [n_facets] each.
 * weight > 0: acc_q += weight q in the same launch.  cell_dofs: the table of c's space in kernel cell order.  One lane per
 * facet, no atomics.  The per-tag sums of fq: ox_outlet_update(..., params = NULL). */
int ox_scalar_flux(int degree, const ox_cells *cells, const int32_t *cell_dofs, int64_t n_facets, const int32_t *facet_rec,
                   const double *c, int nc, int col, double kappa, double weight, double *q, double *fq, double *cbar,
                   double *acc_q, void *stream);
/* The same with a per-cell diffusivity: q[i] = -(kappa + nut[cell] inv_sct) n . gbar, one fused multiply-add for the
 * coefficient.  nut: device [n_cells] in kernel cell order (read-only); inv_sct = 1 / Sc_t >= 0 (0: no turbulent part). */
int ox_scalar_flux_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, int64_t n_facets,
                         const int32_t *facet_rec, const double *c, int nc, int col, double kappa, const double *nut,
                         double inv_sct, double weight, double *q, double *fq, double *cbar, double *acc_q, void *stream);

/* ---- Reacting scalars: mass-action kinetics, split from the transport step (ox_reaction.hip) ----
 * A network of R <= OX_REACT_MAXR reactions between S <= OX_REACT_MAXS species.  At a dof i with the concentrations c:
 *   k_j   = kdof[j] ? kdof[j][i] : k[j]
 *   a_j   = arr[j] >= 0 ? exp(-Ta[j] / c[arr[j]]) : 1          (no guard on c <= 0: a value that is not finite stays in its dof)
 *   r_j   = ((k_j a_j) p_j0) p_j1 ...,   p_js = c_s^order[j][s] by repeated multiplication (orders 0..3; 1 for order 0)
 *   f_s   = sum_j nu[s][j] r_j                                 (j ascending, from 0)
 *   J_st  = sum_j nu[s][j] d_jt,  d_jt = (k_j a_j) prod_s (s == t ? order[j][s] c_s^(order[j][s] - 1) : p_js)
 *                                        [+ (r_j Ta[j]) / (c_t c_t) where t == arr[j]]       (nothing is divided by c otherwise)
 * The record is a HOST structure, copied into the kernel arguments: its tables are lane-uniform scalar loads. */
#define OX_REACT_MAXS 6
#define OX_REACT_MAXR 12
typedef struct {
  int32_t S, R;
  double nu[OX_REACT_MAXS][OX_REACT_MAXR];     /* products - reactants */
  int32_t order[OX_REACT_MAXR][OX_REACT_MAXS]; /* 0..3 */
  double k[OX_REACT_MAXR];
  const double *kdof[OX_REACT_MAXR];           /* device [n] or NULL: the rate coefficient per dof */
  int32_t arr[OX_REACT_MAXR];                  /* the species whose value is the Arrhenius temperature, or -1 */
  double Ta[OX_REACT_MAXR];
} ox_react_net;
/* Species s lives in column col of an interleaved (n, nc) block -- the species of one network usually sit in different
 * blocks of different nc.  src is read once, out (and out2 where not NULL) written once; src, out and out2 may be one
 * block, and several species may share a block (other columns of it are neither read nor written).  held: device [n]
 * bytes or NULL; where held[i] != 0 the species' value at i is written back as it was read (its Dirichlet rows) while it
 * still enters the rates of the others. */
typedef struct {
  const double *src;
  double *out, *out2;
  const uint8_t *held;
  int32_t nc, col;
} ox_react_species;
/* `substeps` steps h = H / substeps of ROS2 (Verwer, Spee, Blom, Hundsdorfer 1999; second order, L-stable) per dof, all
 * in registers, with g = 1 + 1/sqrt(2) and W = I - (g h) J(y):
 *   W k1 = f(y);   W k2 = f(y + h k1) - 2 k1;   y <- (y + (1.5 h) k1) + (0.5 h) k2
 * W is factorised once per substep with partial pivoting (largest |.| of the column, ties to the lower row), the pivots
 * kept as reciprocals; rows are exchanged through selects over compile-time indices.  The step count is fixed: equal inputs
 * give equal bits.  f = 0 and J = 0 (all k_j = 0) leave y bit-unchanged.  One lane per dof, one instantiation per S, no
 * LDS, no atomics, no scratch, no host synchronisation.  species: HOST array [net->S]. */
int ox_scalar_react(const ox_react_net *net, const ox_react_species *species, int64_t n, double H, int substeps,
                    void *stream);
/* rates[j n + i] = r_j at dof i from the species' src blocks (device [R][n]): the rate function of ox_scalar_react alone. */
int ox_reaction_rates(const ox_react_net *net, const ox_react_species *species, int64_t n, double *rates, void *stream);

/* ---- Wall shear stress, traction and boundary forces on exterior facets (ox_wall.hip) ----------
 * Facet i -- the caller passes the facets SORTED by tag -- belongs to the cell at kernel position facet_rec[2 i] and lies
 * opposite that cell's local vertex facet_rec[2 i + 1] (a record outside the tables reads nothing and leaves NaN).  With
 * the outward unit normal n = -grad(lambda_a) / |grad(lambda_a)|, the measure |f| = |det J| |grad(lambda_a)| / (gdim-1)!
 * and the facet means gbar of grad u and pbar of p (exact: compile-time facet means of the basis):
 *   t[i]   = -pbar n + nu_eff (gbar + gbar^T) n,  nu_eff = nu + nut[cell] (nut: device [n_cells] in kernel cell order,
 *            or NULL);   wss[i] = t[i] - (t[i].n) n;   ft[i] = |f| t[i]                (device [n_facets][gdim] each)
 * weight > 0: acc_vec += weight wss, acc_mag += weight |wss| ([n_facets]), acc_t += weight t, in the same launch.
 * u interleaved [n_u][gdim], p [n_q]; cell_vdofs / cell_qdofs: the tables of the velocity component space (degree 1, 2, 3)
 * and the pressure space (P1-P1, P2-P1, P3-P2) in kernel cell order.  One lane per facet, no atomics, fixed order. */
int ox_wall_stress(int u_degree, int p_degree, const ox_cells *cells, const int32_t *cell_vdofs, const int32_t *cell_qdofs,
                   int64_t n_facets, const int32_t *facet_rec, const double *u, const double *p, const double *nut,
                   double nu, double weight, double *t, double *wss, double *ft, double *acc_vec, double *acc_mag,
                   double *acc_t, void *stream);
/* ring[slot][k][:] = -rho sum_{tag_ptr[k] <= i < tag_ptr[k+1]} ft[i]  (the force the fluid exerts on the facets of tag k);
 * ring: device [capacity][n_tags][gdim], tag_ptr: device [n_tags + 1].  One block per tag, a fixed tree: identical inputs
 * give identical bits. */
int ox_wall_forces(int gdim, int n_tags, const int64_t *tag_ptr, const double *ft, double rho, double *ring,
                   int64_t capacity, int64_t slot, void *stream);

/* ---- Outlet models on exterior facets: flow rates, resistance / RCR Windkessel, backflow (ox_outlet.hip, DESIGN.md
 * section 17).  Facets and records as for ox_wall_stress: sorted by tag, facet_rec[2 i] the kernel position of the cell,
 * facet_rec[2 i + 1] the opposite local vertex (a record outside the tables leaves NaN in flux[i]).
 *   flux[i] = |f| n . ubar,  ubar the facet mean of u (exact: compile-time facet means of the P1 / P2 / P3 basis), n outward:
 * a positive flux leaves the domain.  u interleaved [n_u][gdim].  One lane per facet. */
int ox_outlet_flux(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_facets,
                   const int32_t *facet_rec, const double *u, double *flux, void *stream);
/* One block per tag k: Q = sum_{tag_ptr[k] <= i < tag_ptr[k+1]} flux[i] (lane-strided partial sums, a fixed tree) goes to
 * ring[slot][k] (device [capacity][n_tags]).  params == NULL: nothing else.  Otherwise params: device [n_tags][8] =
 * (kind, Rp, C, Rd, p_distal, rho, -, -), kind 0 none / 1 resistance / 2 RCR; state: device [n_tags], the pressure Pc of
 * the capacitor; kind 2 advances it by backward Euler with this Q,
 *   Pc <- (Pc + (dt/C)(Q + p_distal/Rd)) / (1 + dt/(Rd C))       (Rd = 0: Pc <- p_distal),
 * P = Pc + Rp Q, hist[slot][k] = (Q, P, Pc) (device [capacity][n_tags][3]) and h[k * h_stride + dofs[j]] = P / rho for
 * dof_ptr[k] <= j < dof_ptr[k+1]; no other entry of h is written. */
int ox_outlet_update(int n_tags, const int64_t *tag_ptr, const double *flux, double *ring, int64_t capacity, int64_t slot,
                     const double *params, double dt, double *state, double *hist, const int64_t *dof_ptr,
                     const int32_t *dofs, double *h, int64_t h_stride, void *stream);
/* Backflow stabilisation -beta int_Gamma min(u_ab . n, 0) u . v ds, Crank-Nicolson: for row rows[i], over its pairs
 * row_ptr[i] <= k < row_ptr[i+1] -- facet pair_facet[k] (an index into facet_rec / beta, pairs in ascending facet id) on
 * which the row is dof number pair_loc[k] of the facet's dofs (the cell's dofs that live on the facet, ascending) -- and
 * the facet's dofs s:   e = (beta/2) |f| sum_q w_q max(-u_ab(x_q) . n, 0) phi_r(x_q) phi_s(x_q)   (the facet rule: 2 / 4 /
 * 5 Gauss-Legendre points on an edge, that many squared collapsed Gauss-Jacobi points on a triangle, for P1 / P2 / P3),
 *   a_vals[pair_off[k * nfd + s]] += e  (a negative slot is skipped),   b_first[rows[i]][:] -= e u1[dof_s][:].
 * One lane per row, which owns that row of the matrix and of b_first: no atomics, a fixed order of sums. */
int ox_outlet_backflow(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_rows, const int32_t *rows,
                       const int64_t *row_ptr, const int32_t *pair_facet, const int32_t *pair_loc, const int64_t *pair_off,
                       int64_t n_facets, const int32_t *facet_rec, const double *beta, const double *uab, const double *u1,
                       double *a_vals, int64_t a_size, double *b_first, void *stream);

/* ---- Flux and Robin conditions of a scalar group (ox_scalar.hip) ---------------------------------
 * With n outward and kappa_eff whatever diffuses the scalar:   kappa_eff dc/dn = q   (q > 0 enters the domain) and
 *   -kappa_eff dc/dn = (h + beta max(-u_ab . n, 0)) (c - c_inf),   Crank-Nicolson in c.
 * Condition facets: one record per (facet, condition), sorted by facet id and then by the order of the conditions;
 * facet_rec as for ox_outlet_backflow; q, c_inf: device [n_facets][nfd][nc], h: device [n_facets][nfd] -- nodal values at
 * the facet's dofs (the cell's dofs that live on the facet, ascending), interpolated on the facet; beta: device
 * [n_facets].  For row rows[i], over its pairs row_ptr[i] <= k < row_ptr[i+1] (condition facet pair_facet[k], on which the
 * row is dof number pair_loc[k]; pairs in ascending record order), the facet's dofs s and the facet rule (w_q, x_q) of
 * ox_outlet_backflow:   hq = h(x_q) + beta max(-u_ab(x_q) . n, 0),   e = (1/2) |f| sum_q w_q hq phi_r phi_s,
 *   a_vals[pair_off[k * nfd + s]] += e  (a slot outside [0, a_size) is skipped),
 *   b[rows[i]][col] += |f| sum_q w_q (q_col(x_q) + hq c_inf,col(x_q)) phi_r(x_q) - sum_s e c1[dof_s][col].
 * robin == 0: h = beta = 0; pair_off, h, c_inf, beta, uab, c1 and a_vals are not read.  adv == 0: beta = 0; beta and uab
 * are not read.  A pair or a record outside the tables adds nothing; a row outside [0, n_dofs) is not written.  One lane
 * per row, which owns that row of the matrix and of b (device [n_dofs][nc], nc <= 3): no atomics, a fixed order of sums,
 * equal bits for equal inputs. */
typedef struct ox_scalar_bc_args {
  int degree, nc, robin, adv;
  int64_t n_rows;
  const int32_t *rows;       /* [n_rows]                                        */
  const int64_t *row_ptr;    /* [n_rows + 1]                                    */
  const int32_t *pair_facet; /* [n_pairs]                                       */
  const int32_t *pair_loc;   /* [n_pairs]                                       */
  const int64_t *pair_off;   /* [n_pairs][nfd]                                  */
  int64_t n_facets;
  const int32_t *facet_rec;  /* [n_facets][2]                                   */
  const double *q, *h, *c_inf, *beta;
  const double *uab;         /* [n_dofs][gdim]                                  */
  const double *c1;          /* [n_dofs][nc]                                    */
  double *a_vals;
  int64_t a_size;
  double *b;                 /* [n_dofs][nc]                                    */
  int64_t n_dofs;
} ox_scalar_bc_args;
int ox_scalar_boundary(const ox_cells *cells, const int32_t *cell_dofs, const ox_scalar_bc_args *args, void *stream);

/* ---- Drag zones: -sigma(x, |u|) (u - u_t) in the momentum equation (ox_drag.hip) ---------------
 * Porous media (Darcy-Forchheimer), sponge layers that relax to a target field, solids by Brinkman penalisation.  With
 * M_e the mass matrix of cell e on the velocity component space (|e| times the compile-time table of means of
 * phi_i phi_j):   D = sum_e sigma_e M_e,   A += theta D,   b_first += D u_t - (1 - theta) D u_1.
 *
 * ox_drag_sigma: for list entry k, cell e = zone_cells[k] (kernel cell positions; an entry outside the table is skipped):
 *   sigma[e] = alpha[k] + beta[k] |w(x_e)|,   w = uab - ut (ut == NULL: uab) at the centroid x_e;
 * a w that is not finite gives NaN.  No other entry of sigma (device [n_cells], kernel cell order, zero outside the
 * zones) is written.  uab, ut interleaved [n_u][gdim].  One lane per list entry. */
int ox_drag_sigma(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_zone, const int32_t *zone_cells,
                  const double *alpha, const double *beta, const double *uab, const double *ut, double *sigma, void *stream);
/* For every row r of the listed slices (slice_list: device [n_list], slices with a row adjacent to a zone cell and at
 * most lds_width entries per row -- an even number; a wider slice is skipped: the caller launches per width bin of the
 * pattern), over its (cell e, local index i) pairs in the order of space->adj, cells with sigma[e] == 0 skipped, and the
 * cell's dofs j:   m = sigma[e] |e| MASSD[i][j];   acc[adj_pos[pair][j]] += theta m (from 0, in that order);
 *   rb[:] += m w[dof_j][:]   (w: device [n_u][gdim], the caller's u_t - (1 - theta) u_1, or NULL: no right-hand side);
 * then A->vals[slot k of row r] += acc[k] and b_first[r][:] += rb[:].  A row no such cell touches is not written.  A
 * carries the pattern of the space (M, K and A share it); theta in [0.5, 1].  One lane per row, which owns that row of the
 * matrix and of b_first; the accumulator is wave-private LDS (lds_width x 512 B per wave): no atomics, a fixed order of
 * sums, equal bits for equal inputs.  No table beyond sigma and the slice list is read. */
int ox_drag_rows(const ox_cells *cells, const ox_space_info *space, const ox_sell *A, int64_t n_list,
                 const int32_t *slice_list, int lds_width, const double *sigma, double theta, const double *w,
                 double *b_first, void *stream);
/* ft[k][:] = sigma[e] int_e (u - ut) dx for e = zone_cells[k] (exact: the means of the basis are the column sums of the
 * mass table; an entry outside the table leaves NaN); device [n_zone][gdim].  The sums per zone and the ring are
 * ox_wall_forces' (cells sorted by zone, tag_ptr the zones' segments): with rho < 0 there, the force the fluid exerts on
 * the medium, +|rho| sum ft. */
int ox_drag_force_cells(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_zone,
                        const int32_t *zone_cells, const double *sigma, const double *u, const double *ut, double *ft,
                        void *stream);

/* ---- H1 + collectives: mesh-partitioned runs (one process per GPU, RCCL) -------------- */
int ox_comm_unique_id(char *id128);   /* ncclGetUniqueId on rank 0 (broadcast it out of band) */
int ox_comm_create(const char *id128, int rank, int nranks, void **comm_out); /* ncclCommInitRank */
int ox_comm_info(void *comm, int *nranks, int *rank, int *device); /* ncclCommCount / UserRank / CuDevice: what the
                                   communicator itself reports (bench.py's N > 1 line prints it); NULL outputs are skipped */
int ox_comm_destroy(void *comm);
/* Halo plan of one function space on communicator `comm`.  send_idx: device, owned rows to
 * pack, grouped per peer by send_off; ghosts arrive contiguously per peer at
 * x[n_owned + recv_off[p] ...] (the ghost block of a vector is ordered by (owner, global id)). */
int ox_dist_create(void *comm, int rank, int nranks, int n_peers, const int32_t *peers,
                   const int64_t *send_off, const int32_t *send_idx_dev, const int64_t *recv_off,
                   int64_t n_owned, int64_t n_ghost, ox_dist **out);
/* Direct xGMI transport for a plan (alternative to the RCCL calls; `comm` of ox_dist_create may then
 * be NULL).  Every rank creates one uncached window of ox_p2p_window_bytes(nranks, its n_ghost)
 * bytes, hands the 64-byte IPC handle to all ranks out of band, opens theirs, and enables the
 * transport with: rank_wins[nranks] (own window at [rank]), and per peer of the plan the dof offset
 * of THIS rank's block inside the peer's ghost block (the peer's recv_off for this rank) and the
 * peer's n_ghost.  The plan then owns the window and the mappings.  Exchanges wait at most
 * timeout_s for a peer; ox_dist_status reports a time-out (sticky). */
size_t ox_p2p_window_bytes(int nranks, int64_t n_ghost);
int ox_p2p_window_create(size_t bytes, void **win_dev, char *handle64);
int ox_p2p_window_open(const char *handle64, void **win_dev);
int ox_p2p_window_close(void *win_dev);
int ox_p2p_window_free(void *win_dev);
int ox_dist_enable_p2p(ox_dist *d, void *my_win, void *const *rank_wins, const int64_t *peer_recv_off,
                       const int64_t *peer_n_ghost, double timeout_s);
int ox_dist_p2p_timeout(ox_dist *d, double timeout_s); /* change the bound of the peer waits */
/* The plan's distributed mat-vecs: 1 = start the halo exchange, multiply the interior slices while it is in flight, the
 * boundary slices after it has landed; 0 = exchange, then multiply; -1 = the transport's default (overlap on the xGMI
 * windows and the callback transports, off on RCCL plans until the side-stream send/recv has run between two real GPUs).
 * What DOLFINx/PETSc do inside MatMult (reference fracstep.py:453,497,632); never changes a result. */
int ox_dist_set_overlap(ox_dist *d, int overlap);
/* Release protocol of the xGMI-window transport of a plan (after ox_dist_enable_p2p).  conservative = 1 (the DEFAULT):
 * every storing wave of the push kernel fences at system scope behind its payload stores and the flags -- halo and
 * all-reduce -- are system-scope RELEASE stores.  conservative = 0: the fast form (the storing waves only wait for their
 * write-through stores to be acknowledged, ONE system fence by the last block / per all-reduce wave, relaxed flag
 * stores: 32 us instead of ~130 us for the 2.4 MB velocity halo of a 128^3 x 8 rank, 15 us per all-reduce -- figures
 * measured with every rank on ONE device; the form has never crossed a link).  Keep the default until a run between two
 * GPUs has passed the halo self-test, a bit-exact all-reduce and the rehearsal comparison with conservative = 0. */
int ox_dist_set_p2p_release(ox_dist *d, int conservative);
int ox_dist_disable_p2p(ox_dist *d);
int ox_dist_status(const ox_dist *d);
/* Same plan on a caller-supplied transport instead of RCCL (rehearsals on one GPU, other
 * fabrics): halo_cb(user, packed_send_values_dev, ghost_block_dev, ncomp) and
 * allreduce_cb(user, buf_dev, n) are called at the points where ncclSend/ncclRecv and
 * ncclAllReduce would be, after the stream has been drained; both return 0 on success. */
int ox_dist_create_custom(int rank, int nranks, int n_peers, const int32_t *peers,
                          const int64_t *send_off, const int32_t *send_idx_dev, const int64_t *recv_off,
                          int64_t n_owned, int64_t n_ghost,
                          int (*halo_cb)(void *, const double *, double *, int),
                          int (*allreduce_cb)(void *, double *, int), void *user, ox_dist **out);
/* blocking copy helper for such transports: to_device = 1 host->device, 0 device->host */
int ox_memcpy(void *dst, const void *src, size_t bytes, int to_device, void *stream);
int ox_dist_destroy(ox_dist *d);
/* scatter_forward (owner -> ghost) of an interleaved vector (fracstep.py:453,...). */
int ox_halo_forward(const ox_dist *d, double *x, int ncomp, void *stream);
int ox_allreduce_sum(const ox_dist *d, double *buf_dev, int n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
