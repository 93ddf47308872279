"""
Builds the native pieces in-tree (no pip, no JIT cache):
  * ch_shrinkwrap_amd/libnanowrap_hip.so  -- the HIP kernels + C-ABI (hipcc, --offload-arch=gfx950): one object per row of UNITS below
  * ch_shrinkwrap_amd/libnw_remesh.so     -- the block-boundary remesher (host C++, g++; include/nw_remesh.h)
The oracle (test infrastructure) is built by oracle/Makefile, see __graft_entry__.build().
"""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, 'libnanowrap_hip.so')


def _csrc(name):
    return os.path.join(HERE, 'csrc', name)


def _include(name):
    return os.path.join(os.path.dirname(HERE), 'include', name)


# -ffp-contract=off : the parity-critical float32 arithmetic must round products before adding, exactly like
#                     the NumPy reference (explicit fma() is used where contraction is wanted);
# -munsafe-fp-atomics: float/double atomicAdd -> global_atomic_add_f32/f64 (no CAS loop).
HIPCC_FLAGS = ['-O3', '--offload-arch=gfx950', '-fPIC', '-shared', '-ffp-contract=off', '-munsafe-fp-atomics',
               '-fvisibility=hidden', '-Wall', '-Wno-unused-function']
_BASE = ['-O3', '--offload-arch=gfx950', '-fPIC', '-fvisibility=hidden']
# the block-boundary query units: no contraction, as the pairing kernel and the half-edge lengths must round every product as the
# reference's C loop and TriMesh's NumPy do (their results are bit-identical)
_QUERY = _BASE + ['-ffp-contract=off', '-Wall', '-Wno-unused-function']
_BQ_H = [_csrc('nw_bq.h'), _csrc('nw_bq_core.h')]         # (nw_bq.h includes its HIP-free part, nw_bq_core.h)
_BQ = _BQ_H + [_csrc('nw_device.h')]                      # (nw_device.h: nw_wave_incl_scan)

OBJ_MAIN, OBJ_HOLEPUNCH, OBJ_SURGERY, OBJ_BQ = _csrc('nanowrap.o'), _csrc('nw_holepunch.o'), _csrc('nw_surgery.o'), _csrc('nw_bq.o')
OBJ_ISOSURFACE = _csrc('nw_isosurface.o')
OBJ_EVALUATION = _csrc('nw_evaluation.o')
OBJ_SIMULATION = _csrc('nw_simulation.o')
OBJ_DISTANCE = _csrc('nw_distance.o')
OBJ_NEIGHBOURS = _csrc('nw_neighbours.o')
OBJ_INTERSECTIONS = _csrc('nw_intersections.o')
OBJ_RAYS = _csrc('nw_rays.o')
OBJ_VOLUME = _csrc('nw_volume.o')
OBJ_PROXIMITY = _csrc('nw_proximity.o')
OBJ_MAPPING = _csrc('nw_mapping.o')
OBJ_CLUSTERING = _csrc('nw_clustering.o')
OBJ_PAIRS = _csrc('nw_pairs.o')
OBJ_GEODESIC = _csrc('nw_geodesic.o')
OBJ_SKELETON = _csrc('nw_skeleton.o')
OBJ_STRUCTURE = _csrc('nw_structure.o')
OBJ_POISSON = _csrc('nw_poisson.o')
# the translation units of libnanowrap_hip.so: (source, object, what else it is rebuilt for, flags).  The objects are linked in this order.
UNITS = [
    # the per-iteration kernels and the C-ABI; every header of csrc/ but nw_bq.h and nw_bq_core.h is included by it (directly or through
    # nw_kernels.h), nw_host_copy.h among them: the HIP-free host half of the result hand-back, which the tests also compile for the CPU
    (_csrc('nanowrap.hip'), OBJ_MAIN, sorted(set(glob.glob(_csrc('*.h'))) - set(_BQ_H)) + [_include('nanowrap.h')],
     [f for f in HIPCC_FLAGS if f != '-shared']),
    # set-up radix sort (hipCUB)
    (_csrc('nw_sort.hip'), _csrc('nw_sort.o'), [], _BASE + ['-Wno-unused-value']),
    # the block-boundary remesher as kernels (hipCUB scans; nw_remesh_plan.h: what its host driver decides, which the tests also compile
    # for the CPU)
    (_csrc('nw_remesh_dev.hip'), _csrc('nw_remesh_dev.o'), [_include('nanowrap.h'), _csrc('nw_remesh_plan.h')],
     _BASE + ['-ffp-contract=off', '-Wall', '-Wno-unused-value', '-Wno-unused-function']),
    # the hole-punch point queries
    (_csrc('nw_holepunch.hip'), OBJ_HOLEPUNCH, [_include('nw_holepunch.h')] + _BQ_H, _QUERY),
    # the neck / short-edge / inner-surface queries
    (_csrc('nw_surgery.hip'), OBJ_SURGERY, [_include('nw_surgery.h')] + _BQ, _QUERY),
    # the density isosurface of the cloud (the start surface of a fit)
    (_csrc('nw_isosurface.hip'), OBJ_ISOSURFACE, [_include('nw_isosurface.h')] + _BQ_H, _QUERY),
    # the fit-quality metric: mesh sampling and nearest neighbours between two clouds (nw_evaluation_core.h: the sampler's arithmetic,
    # which the tests also compile for the CPU)
    (_csrc('nw_evaluation.hip'), OBJ_EVALUATION, [_include('nw_evaluation.h'), _csrc('nw_evaluation_core.h')] + _BQ_H, _QUERY),
    # the SMLM cloud simulator: a shape's signed distance as a postfix program, the surface lattice, the localization model
    (_csrc('nw_simulation.hip'), OBJ_SIMULATION, [_include('nw_simulation.h')] + _BQ_H, _QUERY),
    # the exact signed distance from points to the mesh (nw_distance_core.h: the point-triangle distance and the pseudonormals, which the
    # tests also compile for the CPU)
    (_csrc('nw_distance.hip'), OBJ_DISTANCE, [_include('nw_distance.h'), _csrc('nw_distance_core.h')] + _BQ_H, _QUERY),
    # the exact k-th-nearest-neighbour distance, for query lists and for the nodes of a voxel lattice (nw_neighbours_core.h: the list of
    # the k best, the ring bound and the quantisation, which the tests also compile for the CPU)
    (_csrc('nw_neighbours.hip'), OBJ_NEIGHBOURS, [_include('nw_neighbours.h'), _csrc('nw_neighbours_core.h')] + _BQ_H, _QUERY),
    # the self-intersection check: which pairs of faces cross (nw_intersections_core.h: the pair predicate, which the tests also compile
    # for the CPU)
    (_csrc('nw_intersections.hip'), OBJ_INTERSECTIONS, [_include('nw_intersections.h'), _csrc('nw_intersections_core.h')] + _BQ_H, _QUERY),
    # ray casting against the mesh: local thickness and the parity side test (nw_rays_core.h: the ray-face test and the walk along the
    # ray, which the tests also compile for the CPU; it uses nw_intersections_core.h's vectors and centroids)
    (_csrc('nw_rays.hip'), OBJ_RAYS, [_include('nw_rays.h'), _csrc('nw_rays_core.h'), _csrc('nw_intersections_core.h')] + _BQ_H, _QUERY),
    # the banded signed-distance volume of the mesh on a voxel lattice (nw_volume_core.h: the node position, the capped walk, the band
    # rule, the predecessor rule and the quantisation, which the tests also compile for the CPU; it includes nw_distance_core.h)
    (_csrc('nw_volume.hip'), OBJ_VOLUME, [_include('nw_volume.h'), _csrc('nw_volume_core.h'), _csrc('nw_distance_core.h')] + _BQ_H, _QUERY),
    # the exact distance between two meshes, per face of one of them (nw_proximity_core.h: the triangle-triangle distance and the capped
    # walk of a face over the other mesh's centroid grid, which the tests also compile for the CPU; it includes nw_distance_core.h and
    # nw_intersections_core.h)
    (_csrc('nw_proximity.hip'), OBJ_PROXIMITY, [_include('nw_proximity.h'), _csrc('nw_proximity_core.h'), _csrc('nw_distance_core.h'),
                                                _csrc('nw_intersections_core.h')] + _BQ_H, _QUERY),
    # what the eleven above share (csrc/nw_bq.h), and the two below them: the exclusive scan, the point grid's bounding box and
    # counting sort, float and double, the cloud query units' cloud grid and the mesh query units' face grid (their arithmetic is in
    # nw_bq_core.h, which nw_neighbours_core.h includes for the cloud point: every unit on that header lists it through _BQ_H)
    (_csrc('nw_bq.hip'), OBJ_BQ, _BQ, _QUERY),
    # localizations mapped onto the mesh: per-vertex mass, per-face counts and value sums as integers (nw_mapping_core.h: the weights, the
    # quantisation, the limbs and the vertex areas, which the tests also compile for the CPU; it includes nw_volume_core.h for the capped
    # walk and through it nw_distance_core.h)
    (_csrc('nw_mapping.hip'), OBJ_MAPPING, [_include('nw_mapping.h'), _csrc('nw_mapping_core.h'), _csrc('nw_volume_core.h'),
                                            _csrc('nw_distance_core.h')] + _BQ_H, _QUERY),
    # DBSCAN clustering of the cloud: neighbour counts, core points, clusters, border points (nw_clustering_core.h: near, the walk, the
    # guard of the two shortcuts and the three visitors, which the tests also compile for the CPU; it includes nw_neighbours_core.h for
    # the squared distance and the ring bound)
    (_csrc('nw_clustering.hip'), OBJ_CLUSTERING, [_include('nw_clustering.h'), _csrc('nw_clustering_core.h'), _csrc('nw_neighbours_core.h')] + _BQ_H,
     _QUERY),
    # pair-distance counts of the cloud: the histogram of pair distances and the same counts per localization (nw_pairs_core.h: the
    # edges, the bin and the walk over a clamped box of cells, which the tests also compile for the CPU; it includes
    # nw_neighbours_core.h for the squared distance and the cell slack)
    (_csrc('nw_pairs.hip'), OBJ_PAIRS, [_include('nw_pairs.h'), _csrc('nw_pairs_core.h'), _csrc('nw_neighbours_core.h')] + _BQ_H, _QUERY),
    # the distance along the mesh: edge and diagonal weights, rounds of relaxations over the half-edges, labels (nw_geodesic_core.h: the
    # weights, the diagonal rule, one relaxation and one label step with the proof that their order is free, which the tests also compile
    # for the CPU; it includes nw_neighbours_core.h for the squared distance)
    (_csrc('nw_geodesic.hip'), OBJ_GEODESIC, [_include('nw_geodesic.h'), _csrc('nw_geodesic_core.h'), _csrc('nw_neighbours_core.h')] + _BQ_H, _QUERY),
    # the level-set skeleton of a mesh: bands of a field, their pieces joined by a union-find over the half-edges, node sums in integers,
    # arcs (nw_skeleton_core.h: the band rule, the piece index, the crossing point, the quantisation and the proof that no sum overflows,
    # which the tests also compile for the CPU; it includes nothing of the project's)
    (_csrc('nw_skeleton.hip'), OBJ_SKELETON, [_include('nw_skeleton.h'), _csrc('nw_skeleton_core.h')] + _BQ_H, _QUERY),
    # the local shape of the cloud: the integer moments of every neighbourhood of radius r, and their covariance's eigenvalues and
    # eigenvectors (nw_structure_core.h: the neighbourhood, the quantisation, the moments with the proof that no sum overflows, the
    # covariance and the Jacobi iteration in a written order, and the walk over a clamped box of cells, which the tests also compile for
    # the CPU; it includes nw_neighbours_core.h for the squared distance and the cell slack)
    (_csrc('nw_structure.hip'), OBJ_STRUCTURE, [_include('nw_structure.h'), _csrc('nw_structure_core.h'), _csrc('nw_neighbours_core.h')] + _BQ_H,
     _QUERY),
    # the screened Poisson grid solver, the comparator of the evaluation: integer splats of an oriented cloud, the system of a level, red-black
    # sweeps, prolongation, the uint64 field (nw_poisson_core.h: a sample's weights, the depth rule, a node's row, one update, the residual,
    # the prolongation and the quantisation with the proofs that no sum overflows, which the tests also compile for the CPU; it includes
    # nothing of the project's)
    (_csrc('nw_poisson.hip'), OBJ_POISSON, [_include('nw_poisson.h'), _csrc('nw_poisson_core.h')] + _BQ_H, _QUERY),
]
DEPS =sorted(set(d for src, _, extra, _ in UNITS for d in [src] + extra))


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build_hip_library(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

    def run(cmd):
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)

    for src, obj, extra, flags in UNITS:
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(d) for d in [src] + extra):
            run([hipcc] + flags + ['-c', '-o', obj, src])
    check_kernel_budgets(verbose=verbose)          # before the link: a kernel that spills or outgrows its occupancy never ships
    run([hipcc, '--offload-arch=gfx950', '-fPIC', '-shared', '-o', LIB] + [obj for _, obj, _, _ in UNITS])
    return LIB


# ---- resource budget of the per-iteration kernels ---------------------------------------------------------------------------------
# The kernels are tuned to an occupancy (waves per SIMD = 512 // VGPRs, capped at 8) that nothing but the register allocator enforces:
# a compiler bump or an innocent edit can spill (scratch > 0: round 2's 20-byte spill of k_nn_wave was only noticed through WRITE_SIZE
# in a profile) or cross a VGPR step and silently halve the waves in flight.  The build reads the gfx950 code object's metadata notes
# (.vgpr_count, .private_segment_fixed_size, .sgpr_spill_count, .group_segment_fixed_size) out of csrc/nanowrap.o and fails on a
# violation; tests/test_abi.py asserts the same numbers.  Budget = (max VGPRs, max LDS bytes); scratch and VGPR spills must be 0.
LLVM_BIN = os.environ.get('NW_LLVM_BIN', '/opt/rocm/lib/llvm/bin')
KERNEL_BUDGETS = {
    # kernel (demangled prefix)       VGPRs  LDS
    'k_nn_wave<false>':               (80, 10 * 1024),     # 6 waves per SIMD (amdgpu_waves_per_eu(6,8)): 12 workgroups of 128 per CU; LDS = the larger of the query's wave-private lists and the appended attraction workgroups' table (9.4 KB)
    'k_attract':                      (72, 20 * 1024),     # 7 workgroups per CU (the run sums keep 24 more registers alive; LDS-pipe-bound: 7 or 8 is the same), 18 KB of LDS each
    'k_face_centroids':               (64, 8 * 1024),
    'k_centroid_scatter':             (64, 0),
    'k_scan_final':                   (64, 1024),
    'k_prior_ring':                   (128, 1024),         # (only launched on its own with NW_RING_IN_NN=0: the ring half rides in the query launch)
    'k_prior_directions':             (96, 1024),          # streaming since the ring half left it: 5 waves per SIMD
    'k_subspace_point_sums':          (128, 1024),         # 4 waves per SIMD cover the launch in one round (rows of two localizations in flight)
    'k_solve_update':                 (128, 1024),
    # the k-d work list of the query (csrc/nw_partition.h): once per cloud, budgeted for zero scratch and against silent growth
    'k_kd_block_max':                 (16, 0),
    'k_kd_seg_counts':                (16, 0),
    'k_kd_fill_segs':                 (32, 0),
    'k_kd_leaf_counts':               (16, 0),
    'k_kd_fill_leaves':               (32, 0),
    'k_kd_partition':                 (64, 146 * 1024),    # two position lists (16 bits) and the composites of 16384 localizations, 512 boxes, a histogram: one workgroup of 1024 per CU
    # hole punching (csrc/nw_holepunch.o): block-boundary queries, budgeted for zero scratch and against silent growth
    'k_hp_empty_faces':               (64, 0),
    'k_hp_pair':                      (64, 8 * 1024),      # two LDS tiles of 256 float4 (centroids, normals)
    'k_hp_prism':                     (176, 0),            # six float64 half-planes and two centres live across the cell walk (3 waves per SIMD)
    'k_hp_cand_geom':                 (32, 0),
    'k_hp_pair_final':                (16, 0),
    # neck removal / short-edge cleanup / inner surfaces (csrc/nw_surgery.o): block-boundary queries, budgeted for zero scratch
    'k_ws_init':                      (16, 0),
    'k_ws_hook':                      (32, 0),
    'k_ws_compress':                  (16, 0),
    'k_ws_number':                    (16, 0),
    'k_ws_stats':                     (64, 0),
    'k_ws_bbox_init':                 (16, 0),
    'k_ws_active':                    (16, 0),
    'k_ws_winding':                   (176, 0),            # eight queries' float64 coordinates and fixed-point sums per thread (2 waves per SIMD)
    'k_ws_lengths':                   (16, 0),
    'k_ws_hist':                      (16, 2048),          # two 256-bin histograms
    'k_ws_pick':                      (32, 0),
    'k_ws_flag':                      (16, 0),
    # the density isosurface (csrc/nw_isosurface.o): set-up kernels, budgeted for zero scratch and against silent growth
    'k_iso_count':                    (16, 16 * 1024),     # the LDS table of voxel ids and counts: 2048 slots of 8 bytes
    'k_iso_widen':                    (16, 0),
    'k_iso_smooth':                   (16, 0),
    'k_iso_hist':                     (16, 1024),          # one 256-bin histogram
    'k_iso_pattern':                  (32, 0),
    'k_iso_compact':                  (16, 0),
    'k_iso_cell_counts':              (16, 0),
    'k_iso_vertices':                 (64, 0),
    'k_iso_quads':                    (32, 0),
    # the fit-quality metric (csrc/nw_evaluation.o): end-of-fit queries, budgeted for zero scratch and against silent growth
    'k_ev_face_setup':                (64, 0),             # the float32 set-up of a face: 23 values live until they are stored
    'k_ev_node_test':                 (32, 0),
    'k_ev_emit':                      (32, 0),
    'k_ev_nearest':                   (64, 64),            # float64 query, best pair and the ring walk's bounds: 8 waves per SIMD; LDS = the four waves' sums
    'k_ev_sum_final':                 (16, 64),
    # the SMLM cloud simulator (csrc/nw_simulation.o): set-up kernels in float64, budgeted for zero scratch (the interpreter's value stack
    # must stay in registers) and against silent growth
    'k_sim_eval':                     (64, 0),             # the interpreter: eight float64 stack slots, the point and the frame: 8 waves per SIMD
    'k_sim_normals':                  (72, 0),
    'k_sim_cell_test':                (64, 0),
    'k_sim_cell_split':               (24, 0),
    'k_sim_leaf_test':                (64, 0),
    'k_sim_leaf_emit':                (32, 0),
    'k_sim_project':                  (72, 0),             # the interpreter seven times a step, the point and the gradient live across them: 7 waves per SIMD
    'k_sim_loc_error':                (32, 0),
    'k_sim_displace':                 (56, 0),             # float64 log and cospi
    'k_sim_background':               (16, 0),
    'k_sim_copy_hist':                (16, 1024),          # one 256-bin histogram
    'k_sim_copy_equal':               (16, 0),
    'k_sim_copy_keep':                (16, 0),
    'k_sim_copy_emit':                (88, 0),             # three normals and three photon draws per copy, unrolled: 5 waves per SIMD
    # the point-to-mesh distance (csrc/nw_distance.o): an end-of-fit query in float64, budgeted for zero scratch and against silent growth
    'k_md_query':                     (128, 64),           # float64 query, best record (d2, d, closest point, face, feature) and one exact test in flight: 4 waves per SIMD; LDS = the four waves' sums
    'k_md_sum_final':                 (16, 64),
    # the k-th-neighbour distance (csrc/nw_neighbours.o): set-up queries in float64, budgeted for zero scratch (a lane's k best live in LDS,
    # never in a register array indexed at run time) and against silent growth
    'k_kn_queries':                   (64, 32 * 1024),     # LDS = 128 lanes x 32 slots x 8 bytes
    'k_kn_nodes':                     (64, 32 * 1024),
    # the self-intersection check (csrc/nw_intersections.o): an end-of-fit query in float64, budgeted for zero scratch (the corners of a
    # shared-vertex pair are picked with selects, never from an array indexed at run time) and against silent growth
    'k_mx_count':                     (168, 0),            # the lane's own face in float64 (ids, corners, centroid, radius), the candidate's, and the predicate's two normals and triple products: 3 waves per SIMD
    'k_mx_emit':                      (168, 0),
    'k_mx_stats':                     (64, 0),             # the walk without the predicate
    'k_mx_totals':                    (24, 128),           # LDS = the four waves' three sums
    # ray casting (csrc/nw_rays.o): an end-of-fit query in float64, budgeted for zero scratch and against silent growth
    'k_rc_first':                     (128, 0),            # the ray, the piece, the candidate's centroid and one exact test in flight: 4 waves per SIMD (some of the walk's uniform values sit in VGPR lanes: no scratch)
    'k_rc_count':                     (128, 0),            # the same walk without the early exit, and the count: 4 waves per SIMD
    'k_rc_totals':                    (24, 96),            # LDS = the four waves' three sums
    # the signed-distance volume (csrc/nw_volume.o): the query's walk with a band, one lane per lattice node; no atomics, zero scratch
    'k_vx_nodes':                     (128, 192),          # k_md_query's record and walk, the band and six counters: 4 waves per SIMD; LDS = the four waves' six counters
    'k_vx_seed':                      (128, 64),           # one exact test in flight; LDS = the four waves' (d2, face)
    'k_vx_sweep':                     (24, 0),
    'k_vx_finish':                    (16, 0),
    'k_vx_totals':                    (32, 192),           # LDS = the four waves' six counters
    # the mesh-to-mesh distance (csrc/nw_proximity.o): the query's walk with a band, one lane per face of the querying mesh; no atomics of its
    # own, zero scratch (the corners of a candidate and of the 3 x 3 edge pairs are picked with selects inside loops that stay loops, never from an array
    # indexed at run time)
    'k_mm_query':                     (168, 160),          # the lane's face (centroid, radius, corner pointers), the walk's cell ranges and (d2, face), both triangles in float64 with their normals and one point-triangle or edge-edge candidate in flight: 3 waves per SIMD (amdgpu_waves_per_eu(3, 8)); LDS = the four waves' five counters
    'k_mm_finish':                    (136, 0),            # one pair test with its kind and two closest points: 3 waves per SIMD
    'k_mm_totals':                    (32, 160),           # LDS = the four waves' five counters
    # localizations on the mesh (csrc/nw_mapping.o): the volume unit's walk with one lane per localization, then integer atomics whose
    # results are not read; zero scratch (the weights are written with constant indices, the corners' atomics are spelled out)
    'k_lm_face_setup':                (64, 0),
    'k_lm_map':                       (128, 96),           # k_vx_nodes' record and walk, the weights and one product's limbs: 4 waves per SIMD; LDS = the four waves' three counters
    'k_lm_totals':                    (32, 96),            # LDS = the four waves' three counters
    # DBSCAN clustering (csrc/nw_clustering.o): one lane per point in cell order, the walk's visitor in registers; zero scratch.  All of them
    # reach 8 waves per SIMD (512 // VGPRs, capped at 8) with room to the next step at 64
    'k_pc_count':                     (56, 64),            # the point in float64, the walk's ranges and two counters: 8 waves per SIMD; LDS = the four waves' two counters
    'k_pc_hook':                      (56, 64),            # the same walk and the two roots of a union: 8 waves per SIMD
    'k_pc_compress':                  (16, 0),
    'k_pc_number':                    (16, 0),
    'k_pc_border':                    (56, 64),            # the same walk and the best (d2, index): 8 waves per SIMD
    'k_pc_stats':                     (40, 96),            # eight values through the wave's butterflies: 8 waves per SIMD; LDS = the four waves' three counters
    'k_pc_totals':                    (64, 256),           # eight 64-bit sums per thread, one workgroup: 8 waves per SIMD; LDS = the four waves' eight counters
    # pair-distance counts (csrc/nw_pairs.o): one lane per query, its counters in a column of LDS, no atomics on the results; zero scratch
    'k_pq_pairs<false>':              (56, 8 * 1024),      # up to 16 bins: 128 lanes x 16 bins x 4 bytes; the edges are scalar operands
    'k_pq_pairs<true>':               (56, 17 * 1024),     # up to 64 bins: 64 lanes x 64 bins x 4 bytes and the LDS copy of the edges (512 bytes)
    'k_pq_totals':                    (24, 2048),          # LDS = one 64-bit sum per thread
    # the distance along the mesh (csrc/nw_geodesic.o): one lane per half-edge or per vertex, 64-bit integer atomics on D; zero scratch.  All
    # of them reach 8 waves per SIMD
    'k_gd_weights':                   (64, 256),           # two corners unfolded in float64 (amdgpu_waves_per_eu(8, 8)); LDS = the workgroup's count
    'k_gd_seed':                      (16, 0),
    'k_gd_relax':                     (32, 256),           # one arc, two distances and a candidate; LDS = the workgroup's vote
    'k_gd_labels':                    (32, 256),
    'k_gd_finish':                    (16, 256),           # LDS = the workgroup's two counts
    'k_gd_totals':                    (24, 2048),          # LDS = one 64-bit sum per thread
    # the level-set skeleton (csrc/nw_skeleton.o): one lane per vertex, face, half-edge or piece; a union-find with compare-and-swaps and
    # 64-bit integer atomic adds whose results are not read; zero scratch (a piece's corners are picked with selects).  All of them are
    # meant to reach 8 waves per SIMD (512 // VGPRs, capped at 8), k_sk_sums with two registers to spare
    'k_sk_bands':                     (32, 512),           # three corners' bands; LDS = the four waves' span sums and largest bands, two votes
    'k_sk_totals':                    (24, 2048),          # LDS = one 64-bit word per thread
    'k_sk_init':                      (16, 0),             # the binary search in piece_start
    'k_sk_hook':                      (32, 0),             # the edge's band range and the two roots of a union
    'k_sk_compress':                  (16, 0),
    'k_sk_number':                    (16, 0),
    'k_sk_sums':                      (64, 0),             # three corners in float64, two crossing points, twelve 64-bit terms
    'k_sk_arcs':                      (16, 0),
    'k_sk_vertex':                    (16, 0),
    # the local shape of the cloud (csrc/nw_structure.o): one lane per query, its ten 64-bit sums in registers, no atomics on the results;
    # zero scratch
    'k_st_moments':                   (64, 64),            # the query in float64, the walk's ranges, ten 64-bit sums (62 VGPRs): 8 waves per SIMD; LDS = the two waves' four counters
    'k_st_eigen':                     (64, 0),             # six elements of C, nine of V and a rotation in flight, all float64 (60 VGPRs): 8 waves per SIMD
    'k_st_totals':                    (24, 2048),          # LDS = one 64-bit sum per thread
    # the screened Poisson grid solver (csrc/nw_poisson.o): one lane per sample, per node or per pair of x-neighbours; 64-bit integer atomics
    # whose results are not read, no float atomics; zero scratch (a node's three coordinates are walked by an unrolled loop).  All of them
    # reach 8 waves per SIMD; LDS = the four waves' partial sums or maxima
    'k_sp_prepare':                   (24, 32),
    'k_sp_mark':                      (32, 0),
    'k_sp_count':                     (16, 32),
    'k_sp_splat':                     (40, 0),             # three axes' two nodes and weights, the normal, one product in flight
    'k_sp_splat_lds':                 (56, 16 * 1024),     # the same over a copy of levels 2 and 3 in LDS (4 planes of 512 nodes) and a loop over the samples
    'k_sp_splat_lds4':                (56, 128 * 1024),    # the same for level 4 (4 planes of 4096 nodes): one workgroup a CU
    'k_sp_system':                    (24, 0),
    'k_sp_prolong':                   (32, 0),             # eight coarse values
    'k_sp_relax':                     (16, 0),             # the stencil of one node: bound by memory, not by registers
    'k_sp_residual':                  (16, 32),
    'k_sp_absmax':                    (8, 32),
    'k_sp_field':                     (24, 32),
    # what the eleven units above share (csrc/nw_bq.o), and nw_mapping.o: the exclusive scan, and the point grid in float (hole punching, and
    # the cloud grid of the four cloud query units: neighbours, clustering, pairs, local shape -- k_bq_scatter_f32 is their one scatter, a
    # sorted point carrying its index) and in double (the metric, the face grid)
    'k_bq_scan_tiles':                (32, 1024),
    'k_bq_scan_bsums':                (32, 1024),
    'k_bq_scan_final':                (32, 1024),
    'k_bq_bbox_f32':                  (32, 0),
    'k_bq_cell_count_f32':            (32, 0),
    'k_bq_scatter_f32':               (32, 0),
    'k_bq_bbox_f64':                  (48, 0),             # six 64-bit keys per thread
    'k_bq_cell_count_f64':            (48, 0),
    'k_bq_scatter_f64':               (16, 0),
    # and the face grid of the six mesh query units (distance, intersections, rays, volume, proximity, mapping): a face's float64 centroid and radius
    'k_bq_face_setup':                (56, 0),
    'k_bq_rho_reduce':                (24, 64),            # LDS = the four waves' maxima and sums
}
BUDGETED_OBJECTS = [OBJ_MAIN, OBJ_HOLEPUNCH, OBJ_SURGERY, OBJ_ISOSURFACE, OBJ_EVALUATION, OBJ_SIMULATION, OBJ_DISTANCE, OBJ_NEIGHBOURS, OBJ_INTERSECTIONS, OBJ_RAYS, OBJ_VOLUME, OBJ_PROXIMITY, OBJ_MAPPING, OBJ_CLUSTERING, OBJ_PAIRS, OBJ_GEODESIC, OBJ_SKELETON, OBJ_STRUCTURE, OBJ_POISSON, OBJ_BQ]


def kernel_resources(obj=None):
    """{demangled kernel name: {'vgpr', 'sgpr', 'scratch', 'lds', 'vgpr_spill', 'sgpr_spill'}} of the gfx950 code object inside `obj`
    (default: every object of BUDGETED_OBJECTS, merged)."""
    import re
    import tempfile
    if obj is None:
        out = {}
        for o in BUDGETED_OBJECTS:
            out.update(kernel_resources(o))
        return out
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, 'fat.bin'), os.path.join(td, 'dev.co')
        subprocess.check_call(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat])
        subprocess.check_call([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fat,
                               '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co])
        notes = subprocess.check_output([os.path.join(LLVM_BIN, 'llvm-readelf'), '--notes', co]).decode()
    out = {}
    for entry in re.split(r'\n\s+- \.agpr_count', notes)[1:]:
        def field(f, default='0'):
            m = re.search(r'\.%s:\s+(\S+)' % f, entry)
            return m.group(1) if m else default
        sym = field('name', '')
        if not sym:
            continue
        # demangled by hand (no c++filt dependency): _Z<len><name>[I L b <0|1> E E]... -> name, name<false>, name<true>
        m = re.match(r'_Z(\d+)', sym)
        name = sym
        if m:
            n0 = m.end()
            name = sym[n0:n0 + int(m.group(1))]
            t = re.match(r'ILb([01])EE', sym[n0 + int(m.group(1)):])
            if t:
                name += '<true>' if t.group(1) == '1' else '<false>'
        out[name] = {'vgpr': int(field('vgpr_count')), 'sgpr': int(field('sgpr_count')), 'scratch': int(field('private_segment_fixed_size')),
                     'lds': int(field('group_segment_fixed_size')), 'vgpr_spill': int(field('vgpr_spill_count')), 'sgpr_spill': int(field('sgpr_spill_count'))}
    return out


def check_kernel_budgets(obj=None, verbose=False):
    """Raise RuntimeError if a budgeted kernel is missing, uses scratch, spills VGPRs, or exceeds its VGPR / LDS budget."""
    res = kernel_resources(obj)
    bad = []
    for k, (max_vgpr, max_lds) in KERNEL_BUDGETS.items():
        r = res.get(k)
        if r is None:
            bad.append('%s: not in the code object' % k)
            continue
        if verbose:
            print('  %-28s %3d VGPRs (<= %3d)  %5d B LDS (<= %5d)  scratch %d' % (k, r['vgpr'], max_vgpr, r['lds'], max_lds, r['scratch']))
        if r['scratch'] or r['vgpr_spill']:
            bad.append('%s: %d bytes of scratch, %d VGPRs spilled' % (k, r['scratch'], r['vgpr_spill']))
        if r['vgpr'] > max_vgpr:
            bad.append('%s: %d VGPRs, budget %d' % (k, r['vgpr'], max_vgpr))
        if r['lds'] > max_lds:
            bad.append('%s: %d bytes of LDS, budget %d' % (k, r['lds'], max_lds))
    if bad:
        raise RuntimeError('kernel resource budget violated:\n  ' + '\n  '.join(bad))
    return res


HOST_LIB = os.path.join(HERE, 'libnw_remesh.so')
HOST_SRC = os.path.join(HERE, 'csrc', 'remesh.cpp')
HOST_DEPS = [HOST_SRC, os.path.join(os.path.dirname(HERE), 'include', 'nw_remesh.h')]
HOST_FLAGS = ['-O2', '-std=c++14', '-fPIC', '-shared', '-fvisibility=hidden', '-ffp-contract=off', '-Wall', '-pthread']


def build_host_library(force=False, verbose=False):
    if not force and os.path.exists(HOST_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(HOST_LIB) for d in HOST_DEPS):
        return HOST_LIB
    cmd = [os.environ.get('CXX', 'g++')] + HOST_FLAGS + ['-o', HOST_LIB, HOST_SRC]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return HOST_LIB


if __name__ == '__main__':
    build_hip_library(force=True, verbose=True)
    build_host_library(force=True, verbose=True)
