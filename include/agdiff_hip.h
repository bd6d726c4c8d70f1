/*
 * agdiff_hip.h -- C ABI of libagdiff_hip.so: the MI355X (gfx950) kernels behind the AGDIFF
 * diffusion-sampling hot path.
 *
 * The reference (ADicksonLab/AGDIFF) is pure Python; the native work on this path is done by
 * third-party packages it calls (torch_cluster / torch_scatter / torch_sparse / PyG) and by
 * ATen.  Each entry point below names the reference call site(s) it replaces
 * (paths relative to the reference tree).  All pointers are DEVICE pointers unless marked
 * [host]; all tensors are dense, row-major; indices are int32 on this side of the boundary
 * (the Python host converts from/to the reference's int64).  Every function enqueues work on
 * `stream` (a hipStream_t passed as void*) and returns 0, or a negative agdiff_status code
 * after validating its arguments on the host.  Nothing here allocates, frees or synchronises -- with one exception, named at
 * its entry: agdiff_ring_coords copies its ring sizes back to the host and waits for `stream` before it launches.
 *
 * Struct fields are only `void*`-sized pointers, int64_t, int32_t and float so that the
 * Python binding (agdiff_amd/_lib.py) can mirror them mechanically by parsing this header.
 */
#ifndef AGDIFF_HIP_H
#define AGDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGDIFF_ABI_VERSION 48
#define AGDIFF_HIDDEN 128          /* config.hidden_dim; InteractionBlock.lin hard-codes 256 = 2*128 (schnet.py:190) */
#define AGDIFF_MAX_CONVS 8         /* >= config.num_convs (6) */
#define AGDIFF_MAX_CONVS_LOCAL 8   /* >= config.num_convs_local (4) */
#define AGDIFF_NUM_EDGE_TYPES 100  /* rows of bond_emb (edge.py:49) */
#define AGDIFF_MAX_ATOMS_PER_GRAPH 512   /* most atoms per molecule of the LDS graph build (k_graph) and of agdiff_sampler_front */
#define AGDIFF_MAX_ATOMS_LARGE 16384     /* most atoms per molecule at all (agdiff_graph_build_large).  The large build keeps nothing per
                                            molecule in LDS and its offsets are the batch's (32-bit: checked per batch by the host), so
                                            no size is a hard wall; the bound is set by cost: the build tests all n^2 pairs of a molecule
                                            (at 16384 atoms 2.7e8 per pass; measured: 3.1 ms for 16 x 4096 atoms, the same pair count), the
                                            molecule's positions (12 B per atom: 192 KB) still sit in one XCD's 4 MB L2 next to the lists
                                            being written, and the host's per-molecule work stays in seconds.  Larger systems want a cell
                                            list, which this rule (first 33 candidates in INDEX order) does not map onto. */
#define AGDIFF_RADIUS_CAP 33       /* max_num_neighbors + 1 (torch_cluster.radius_graph, common.py:217) */
#define AGDIFF_TILE 16             /* edges / nodes per MFMA tile */
#define AGDIFF_MAX_CHUNK_TILES 8   /* most tiles one wave walks per chunk in the fused CFConv kernel (128 edges) */
#define AGDIFF_RMSD_MAX_ATOMS 256  /* most (heavy) atoms per conformer in agdiff_rmsd_matrix / agdiff_rmsd_self */
#define AGDIFF_PRUNE_MAX_CONFS 4096 /* most conformers of agdiff_leader_prune: one wave holds the kept set, 64 lanes x 64 bits */
#define AGDIFF_KMEDOIDS_MAX_DIST 4096 /* agdiff_kmedoids: a matrix entry above this (or not >= 0) counts as this far: 2^40 in fixed point */
#define AGDIFF_KMEDOIDS_MAX_ITER 128 /* most updates agdiff_kmedoids may be asked for: it enqueues three launches for each */
#define AGDIFF_KMEDOIDS_WORK_BYTES 131072 /* the scratch agdiff_kmedoids is handed: control words and one 64-bit key per conformer */
#define AGDIFF_SILHOUETTE_WORK_BYTES 65536 /* the scratch agdiff_silhouette is handed: control words and one 64-bit integer per conformer */
#define AGDIFF_PAM_MAX_SWAPS 256 /* most swaps one agdiff_pam_swap call may be asked for: it enqueues three launches for each */
#define AGDIFF_PAM_WORK_BYTES 135168 /* the scratch agdiff_pam_build / agdiff_pam_swap are handed: control words, three 64-bit and two 32-bit words per conformer */
#define AGDIFF_LINKAGE_SINGLE 0 /* agdiff_linkage: the pair weight of two clusters is the minimum over their pairs */
#define AGDIFF_LINKAGE_COMPLETE 1 /* ... the maximum */
#define AGDIFF_LINKAGE_AVERAGE 2 /* ... the sum, and the key its mean (UPGMA) */
#define AGDIFF_LINKAGE_WORK_FIXED_BYTES 131072 /* agdiff_linkage's scratch is 8 G G bytes + this: control words and 28 bytes per slot, then the uint64 square */
#define AGDIFF_LINKAGE_CUT_WORK_BYTES 65536 /* the scratch agdiff_linkage_cut is handed: control words and one 64-bit key per conformer */
#define AGDIFF_TFD_MAX_COLUMNS 512/* most dihedral columns per conformer in agdiff_tfd_matrix: 32 rows of them are 64 KB of LDS */
#define AGDIFF_RING_MAX_ATOMS 32 /* most atoms of one ring of agdiff_ring_coords (the fewest: 4) */
#define AGDIFF_CLASH_SLICE 256 /* atoms per workgroup of agdiff_clash_scan, and per LDS tile of the atoms it walks (4 KB) */
#define AGDIFF_PLANAR_MAX_ATOMS 8 /* most atoms of one planar group of agdiff_planar_groups: a double bond with three neighbours at
                                     each end (planarity.py's rules give no more; an aromatic ring has 5 or 6) */
#define AGDIFF_RELAX_MAX_ATOMS 1024 /* most atoms per conformer of agdiff_relax_bounds: two fp64 position buffers (48 KB) and the radii
                                       (4 KB) fit the 64 KB of static LDS */
#define AGDIFF_RELAX_MAX_ITERS 10000 /* most updates agdiff_relax_bounds may be asked for */
#define AGDIFF_FLATTEN_MAX_GROUPS 192 /* most planar groups of agdiff_relax_planar: one group per thread of the 256, and six fp64 per
                                         group in LDS (9 KB) next to agdiff_relax_bounds' 52 KB -- 61 KB of the 64 KB of static LDS;
                                         256 groups would not fit */
#define AGDIFF_RESTRAIN_MAX_ATOMS 1024 /* most restrained atoms of ONE graph in agdiff_restrain_pairs: a sweep's new values wait in LDS
                                          (12 KB of fp32) until every read of the sweep is done */
#define AGDIFF_MMD_MAX_CONFS 8192 /* most reference + generated conformers of agdiff_mmd_single: one column of them is 32 KB of LDS */
#define AGDIFF_POLY_MAX_KT 4      /* most 32-term k-tiles of the radius-edge filter polynomial (degree 127): 1, 2 what smooth
                                      checkpoints take; 3, 4 the rungs between them and the filter MLPs for sharp ones */
#define AGDIFF_POLY_MAX_SLOTS 16   /* most local edge types with filter polynomials; the first sets that fit stay in LDS next to the
                                      radius edges' set (5 at poly_kt 1), the others are read from L2 by the tiles that meet them */
#define AGDIFF_RAD_STRIDE 48       /* rows reserved per target in the radius-edge list (three 16-row tiles >= AGDIFF_RADIUS_CAP) */

enum agdiff_status {
  AGDIFF_OK = 0,
  AGDIFF_ERR_ARG = -1,       /* null pointer / negative size / inconsistent sizes */
  AGDIFF_ERR_LIMIT = -2,     /* a compile-time limit above is exceeded */
  AGDIFF_ERR_LAUNCH = -3     /* hipGetLastError() after a launch */
};

/* ---- packed network weights (built by agdiff_amd/packing.py from the reference state_dict) ---
 * "pk" = MFMA-operand-major packing of a Linear weight W[out][in] in 2-KiB blocks of 16 outputs x 32 inputs
 * (OT = ceil(out/16), KT = ceil(in/32), zero padded), blocks ordered [OT][KT]; "pkk" = the same blocks in
 * k-tile-outer order [KT][OT], for layers whose input is streamed in 32-feature k-tiles.  Lane l of block
 * (ot, t) holds the eight weights W[16*ot + (l&15)][32*t + c], c in {4q..4q+3, 16+4q..16+4q+3}, q = l>>4:
 *   precision 0: two 16-byte units [u][lane][4 fp32] (elements 4u..4u+3)
 *   precision 1: two 16-byte units [part][lane][8 bf16], part 0 = bf16(w), part 1 = bf16(w - hi)
 *   precision 2: the same with fp16 (agdiff_params_t.precision_local)
 * Dimensions in the field comments below are [OT][KT] block counts.  Vectors are in natural feature order. */
typedef struct agdiff_conv_params {
  /* CFConv filter networks of one InteractionBlock (schnet.py:169-186), conv1 (F=128) and conv2 (F=64) fused.
   * ShiftedSoftplus (schnet.py:71-80) is evaluated in base 2 with its constants folded into the two linear
   * layers by the host: with c = beta * log2(e) per conv, layer 1 yields u = c (W1 a + b1); the kernel forms
   * s = max(u, log2(1 + 2^u)); since softplus(beta x) - ln 2 = ln 2 (s - 1), layer 2 uses ln 2 * W2 and
   * b2 - ln 2 * W2 1.  Precision 1 (split-bf16) keeps the shift out of the bias: layer 1 yields u' = u - 1, the
   * kernel forms s - 1 = max(u', log2(1/2 + 2^u')) -- the operand whose 16 bits the filter gets -- and layer 2 uses b2. */
  const float* filt_w1_pk;   /* pkk [4][12]: rows 0..127 c1 * conv1.nn.0.weight, 128..191 c2 * conv2.nn.0.weight */
  const float* filt_b1;      /* [192] c * nn.0.bias (split-bf16: minus 1, the kernel then forms s - 1 instead of s) */
  const float* filt_w2a_pk;  /* pk [8][4]: ln2 * conv1.nn.2.weight */
  const float* filt_w2b_pk;  /* pk [4][2]: ln2 * conv2.nn.2.weight */
  const float* filt_b2;      /* [192] nn.2.bias - ln2 * rowsum(nn.2.weight) (split-bf16: nn.2.bias) */
  const float* dist_seg;     /* [2][100]: DistanceWeightingNetwork (schnet.py:83-100) of conv1 / conv2 by segments: the network's
                                pre-sigmoid value layer2(relu(layer1(d))) is piecewise linear in d with at most 32 kinks
                                (d = -b1_k / w1_k); bp[32] = the kinks in ascending order (padded with +inf), then
                                alpha[33], beta[33] with value = alpha[s] d + beta[s] on segment s = #{kinks <= d}, summed
                                over the active hidden units in float64 by the host; [98..99] unused */
  /* node side of the block (schnet.py:153-158, 201-216, 219-234) */
  const float* lin1_pk;      /* pk [12][4]: BN-folded conv1.lin1 (rows 0..127) and conv2.lin1 (128..191) */
  const float* lin1_b;       /* [192] */
  /* InteractionBlock.act (ShiftedSoftplus with learnable beta, schnet.py:71-80,206) is evaluated in base 2 like the filter
   * networks' one: kb = act.beta * log2(e) is folded into lin2 (u = kb (W2 agg + b2)), the kernel forms
   * s = max(u, log2(1 + 2^u)), and lin takes ln2 * W with bias b - ln2 * W 1  (softplus(beta x) - ln 2 = ln 2 (s - 1)) */
  const float* lin2a_pk;     /* pkk [4][8]: kb * BN-folded conv1.lin2 */
  const float* lin2b_pk;     /* pkk [2][8]: kb * BN-folded conv2.lin2 */
  const float* lin2_b;       /* [256] kb * (BN-folded biases) */
  const float* lin_pk;       /* pk [8][8]: ln2 * InteractionBlock.lin (256->128) */
  const float* lin_b;        /* [128] lin.bias - ln2 * rowsum(lin.weight) */
  const float* gate1_pk;     /* pk [4][4]: attention.0 (128->64) */
  const float* gate1_b;      /* [64] */
  const float* gate2_w;      /* [64]  attention.2 */
  const float* scale1_pk;    /* pk [1][4]: scaling fc.0 (128->8, rows 8..15 zero) */
  const float* scale2_pk;    /* pk [8][1]: scaling fc.2 (8->128, cols 8..31 zero) */
  const float* filt_poly_pk; /* pk [12][poly_kt] or null: the whole filter network of a RADIUS edge (type 0, d < cutoff) as a
                                polynomial in d -- see agdiff_params_t.poly_kt.  Rows 0..127 conv1, 128..191 conv2; nn.2.bias
                                is the constant term */
  const float* filt_poly_typed_pk; /* [poly_num_slots] x pk [12][poly_kt] or null: the same for the LOCAL edge types that have
                                a slot (agdiff_params_t.poly_type_slot), d in [0, cutoff] (beyond it the CFConv's cutoff factor
                                C(d) is exactly 0, schnet.py:140-146) */
  float gate2_b;
  float act_beta;            /* InteractionBlock.act.beta (informational: folded into lin2 / lin above) */
  float filt_poly_unscale;   /* 2^-S (1 when unused): filt_poly_pk and filt_poly_typed_pk hold 2^S times the coefficients and
                                agdiff_cfconv_node multiplies a target's finished sums by 2^-S -- exact, and it lifts the lo
                                parts of small split-fp16 coefficients out of fp16's subnormal range (quantum 6e-8, i.e. up
                                to 1e-6 of a filter of size 0.2 over 32 terms); the host picks S with max |c| 2^S <= 1024 */
  float pad0;
} agdiff_conv_params_t;

typedef struct agdiff_gin_params {
  const float* w1_pk;        /* pk [8][4] convs.k.nn.layers.0 */
  const float* b1;           /* [128] */
  const float* w2_pk;        /* pk [8][4] BN-folded convs.k.nn.layers.1 */
  const float* b2;           /* [128] */
  float one_plus_eps;
  int32_t relu_out;          /* 1 for all but the last layer (gin.py:134) */
} agdiff_gin_params_t;

/* agdiff_head_params_t.act: torch.nn.functional names the heads' MultiLayerPerceptron may be built with (models/common.py:62-66) */
#define AGDIFF_ACT_RELU 0
#define AGDIFF_ACT_GELU 1        /* erf form (F.gelu default) */
#define AGDIFF_ACT_SILU 2
#define AGDIFF_ACT_TANH 3
#define AGDIFF_ACT_SIGMOID 4
#define AGDIFF_ACT_SOFTPLUS 5    /* beta 1, threshold 20 */
#define AGDIFF_ACT_LEAKY_RELU 6  /* negative_slope 0.01 */
#define AGDIFF_ACT_ELU 7         /* alpha 1 (F.celu with its default alpha is the same function) */
#define AGDIFF_ACT_RELU6 8
#define AGDIFF_ACT_HARDTANH 9    /* [-1, 1] */
#define AGDIFF_ACT_SELU 10
#define AGDIFF_ACT_MISH 11
#define AGDIFF_ACT_HARDSWISH 12
#define AGDIFF_ACT_HARDSIGMOID 13
#define AGDIFF_ACT_SOFTSIGN 14
#define AGDIFF_ACT_LOGSIGMOID 15
#define AGDIFF_ACT_HARDSHRINK 16  /* lambd 0.5 */
#define AGDIFF_ACT_SOFTSHRINK 17  /* lambd 0.5 */
#define AGDIFF_ACT_RRELU 18       /* as evaluated (training=False): negative slope (1/8 + 1/3) / 2 */
typedef struct agdiff_head_params {
  const float* w1_pk;        /* pkk [8][8] layers.0 (256->128) */
  const float* b1;           /* [128] */
  const float* w2_pk;        /* pk [4][4] layers.1 (128->64) */
  const float* b2;           /* [64] */
  const float* w3;           /* [64]  layers.2 */
  const float* attr_poly_pk; /* pkk [poly_kt][8] or null: layers.0.weight[:, 128:] @ edge_attr(d, type 0) as a polynomial in d
                                (agdiff_params_t.poly_kt) */
  float b3;
  int32_t act;               /* AGDIFF_ACT_*: config.mlp_act, the activation between the head's layers (models/common.py:62-66:
                                getattr(F, name); the shipped configs: relu) */
  int32_t precision;         /* as agdiff_params_t.precision, or 2 (split-fp16: only with attr_rows) */
  int32_t pad0;
  int32_t* range_rows;       /* as agdiff_ws_t.range_rows (the head's hidden layer; an edge flags its source node), or null.
                                agdiff_score_forward passes the workspace's */
} agdiff_head_params_t;

typedef struct agdiff_params {
  /* MLPEdgeEncoder (edge.py:84-103), attention dropped (softmax over a size-1 axis == 1) and
   * edge_feature_mlp.2 folded into combination_mlp.0 */
  const float* ee_fe_w;      /* [128] feature_expansion.weight[:,0] */
  const float* ee_fe_b;      /* [128] */
  const float* ee_t1;        /* [100][128]: edge_feature_mlp.0.weight[:,128:] @ bond_emb[t] + bias */
  const float* ee_w1_pk;     /* pk [8][4]: edge_feature_mlp.0.weight[:,:128] */
  const float* ee_t3;        /* [100][128]: comb.0.weight[:,128:] @ bond_emb[t] + comb.0.bias + comb.0.weight[:,:128] @ efm.2.bias */
  const float* ee_w23_pk;    /* pk [8][4]: comb.0.weight[:,:128] @ edge_feature_mlp.2.weight */
  const float* ee_w4_pk;     /* pk [8][4]: combination_mlp.2 */
  const float* ee_b4;        /* [128] */
  /* GaussianSmearingEdgeEncoder (edge.py:17-42 with GaussianSmearing, schnet.py:18-27): used instead of the
   * ee_* fields when edge_encoder == 1; out = [exp(coeff (d - offset_k)^2), k < 64 | bond_emb[type]] */
  const float* ge_offset;    /* [64] rbf.offset buffer = linspace(0, 2 cutoff, 64) */
  const float* ge_emb;       /* [100][64] bond_emb.weight */
  const float* schnet_emb;   /* [100][128] encoder_global.embedding (max_norm renorm applied to used rows) */
  const float* gin_emb;      /* [100][128] encoder_local.node_emb */
  const int32_t* poly_type_slot; /* [100] or null: slot of an edge type in filt_poly_typed_pk, -1 = none */
  const float* dist_union;   /* [K + S * 2 * 2 num_convs] or null (K = dist_union_kinks, S = dist_union_segments below): the
                                DistanceWeightingNetworks of all CFConvs (conv[k].dist_seg) over their COMMON segments on [0, cutoff]:
                                [0..K-1] the union of their kinks in (0, cutoff] ascending (+inf padded; K a power of two > their
                                number, at most 512), then for union segment u = number of those kinks <= d and scale
                                cc = 2 k + (0: conv1, 1: conv2) the line (alpha, beta) at [K + (u * 2 num_convs + cc) * 2]: the same
                                floats dist_seg selects for a d in [0, cutoff], found with ONE search instead of one per conv
                                (agdiff_sampler_front; beyond the cutoff the envelope makes every scale exactly 0) */
  const float* attr_poly_typed_pk; /* [poly_num_slots + attr_poly_far_slots] x pk [8][1] or null: edge_attr itself (128 features) of a
                                local edge of a slotted type as a polynomial in d on [0, cutoff] (agdiff_local_edge_rows); then, for
                                the first attr_poly_far_slots slots, the same on [cutoff, attr_poly_far_hi] (below) */
  agdiff_conv_params_t conv[AGDIFF_MAX_CONVS];
  agdiff_gin_params_t gin[AGDIFF_MAX_CONVS_LOCAL];
  agdiff_head_params_t head_global;
  agdiff_head_params_t head_local;
  int32_t num_convs;
  int32_t num_convs_local;
  float cutoff;
  int32_t smooth;            /* config.smooth_conv */
  int32_t precision;         /* 0: exact fp32 MFMA; 1: split-bf16 (hi+lo, 3 MFMA passes, fp32 accumulate); 2: split-fp16 (the same scheme
                                on v_mfma_f32_16x16x32_f16: 11 + 11 mantissa bits per operand at the same rate; operands beyond
                                fp16's range saturate) -- selects both the kernels and the layout of every packed matrix and
                                of e_attr / l_attr */
  int32_t edge_encoder;      /* config.edge_encoder: 0 'mlp' (edge.py:45-103), 1 'gaussian' (edge.py:17-42) */
  float ge_coeff;            /* -0.5 / (offset[1] - offset[0])^2 (schnet.py:22) */
  int32_t poly_num_slots;    /* 0, or 1..AGDIFF_POLY_MAX_SLOTS: local edge types whose CFConv filters are d-polynomials too
                                (the types the host has met in batches so far and whose fit it accepted); 0 sends the local
                                edges through the filter MLPs.  A batch that brings a type without a slot (fit refused, or more
                                than AGDIFF_POLY_MAX_SLOTS types) runs MIXED: the slotted types' edges by polynomials inside
                                agdiff_cfconv_node, the others through agdiff_cfconv_local (topo->local_type_mask tells) */
  int32_t precision_local;   /* arithmetic of the LOCAL branch's MFMA kernels (GIN layers, local head, local edge_attr rows by
                                polynomial): 0 / 1 as `precision`, 2: split-fp16 (hi + lo fp16, three passes of
                                v_mfma_f32_16x16x32_f16: ~2^-20 per product (both parts truncated: one-sided) at the split-bf16 rate) -- gin[].w*_pk, head_local.w*_pk
                                and attr_poly_typed_pk are packed in THIS mode; the encoder MLP of flagged tiles stays in
                                `precision` */
  int32_t poly_kt;           /* 0: off.  1..AGDIFF_POLY_MAX_KT: radius edges (type 0: no bond embedding; d < cutoff by
                                construction) take their CFConv filters and the edge_attr half of the global head's first layer
                                from polynomials in d instead of the encoder + filter MLPs: both are smooth functions of the ONE
                                scalar d (edge.py:84-103 -> schnet.py:169-179), fitted by the host in float64 at Chebyshev nodes
                                and accepted only when they reproduce the networks to <= 1e-6 of the largest value on a dense
                                grid (agdiff_amd/packing.py).  K = 32 poly_kt terms in the product basis
                                  phi[8 g + j](x) = T_{8 g}(x) T_j(x),  x = 2 d / cutoff - 1,  g < 4 poly_kt,  j < 8
                                (T_n = Chebyshev polynomials; spans all polynomials of degree < K); operand element j of lane
                                quarter q in k-tile t is phi[8 (4 t + q) + j], and the packed blocks are ordered to match. */
  int32_t poly_plan;         /* passes of the split arithmetic over the filter polynomials' terms in agdiff_cfconv_node (0 when
                                precision == 0).  0: every term three passes (hi hi, lo hi, hi lo).  1: the HIGH terms -- f >= 16
                                at poly_kt 1, f >= 32 at poly_kt 2..4 -- take ONE pass (hi x hi): the host sets it only when
                                  fit error + eps1 * max_out sum_{high f} |c[out][f]| <= 1e-6 of the largest filter value
                                for the radius set and the common local types (|phi_f| <= 1; eps1 = 1.5 * 2^-10 split-fp16, 2^-7 split-bf16: the
                                two operand roundings of a single product), agdiff_amd/packing.py poly_pass_plan.
                                  poly_kt 1: TWO MFMAs per 16-channel tile instead of three -- unit 1 of every block of
                                  conv[].filt_poly_pk / filt_poly_typed_pk then holds, for lanes 0..31, their hi elements again
                                  and, for lanes 32..63, the LO elements of lane - 32 (same row, terms 8 (q - 2) + j), and the
                                  kernel's second operand is [lo(phi_f), f < 16 | hi(phi_f), f < 16]: both cross terms of the
                                  low 16 terms in one K = 32 instruction.
                                  poly_kt >= 2: k-tile 0 three passes, the others one (unit 1 of their blocks is not read);
                                  the high terms are then f >= 32.
                                2 (poly_kt >= 3) / 3 (poly_kt 4): k-tiles 0..1 / 0..2 three passes, the others one -- the high terms
                                are f >= 64 / 96: sharp networks whose terms 32..63 (..95) still carry too much weight for plan 1. */
  int32_t tune_cfconv_quad_tiles;    /* [0] agdiff_cfconv_node on quads (topo->group_targets == 4): radius rows in quad tiles too -- quarter k
                                        of a tile = four rows of the quad's k-th target, one set of sums per lane, no exchange between
                                        the quarters (k_cfconv_quad); -1: every target its own radius tiles (k_cfconv_node) */
  /* Kernel-variant thresholds: batch-size crossovers measured on MI355X.  0 selects the library default in
   * brackets; tests set them to reach every variant on small fixtures, agdiff_ws_t.variant_log reports what ran. */
  int64_t poly_slot_mask[2]; /* bit t of the 128-bit mask: edge type t has a slot in poly_type_slot */
  int64_t tune_share_rows_min_nodes;  /* [8192] batches with at least this many atoms take the local edges' edge_attr rows from
                                         the global encoder pass (ws->e_loc) instead of a pass over the canonical local list */
  int64_t tune_node_ldsw_min_tiles;   /* [1536] node stage / GIN layer: from this many 16-node tiles on, workgroups share the
                                         weights through LDS; below, every wave streams them from L2 */
  int64_t tune_node_split_max_tiles;  /* [320] node stage: up to this many tiles four waves share one tile (-1: never) */
  int32_t tune_serial_branches;       /* [0] 1: local and global branch on the caller's stream, no side stream */
  int32_t tune_local_poly_off;        /* [0] 1: local edges through the filter MLPs even when every type has a polynomial */
  int32_t tune_attr_poly_off;         /* [0] 1: agdiff_local_edge_rows evaluates the encoder MLP for every tile */
  int32_t tune_poly_lds_sets;         /* [0 = as many as fit in 160 KiB] agdiff_cfconv_node: at most this many coefficient sets in
                                         LDS, the radius edges' one included (1: every local type's set is read from L2) */
  int32_t attr_poly_far_slots; /* 0, or the number of FAR sets that follow the poly_num_slots near sets in attr_poly_typed_pk: edge_attr
                                  of a local edge type on [cutoff, attr_poly_far_hi].  Local edges LONGER than the cutoff -- bonded
                                  atoms far apart at high sigma, every local edge of a local-only step early in the schedule --
                                  then take their rows from it instead of the encoder MLP (beyond the cutoff the encoder's GELUs are
                                  saturated: a 32-term fit on [rc, 10 rc] is good to ~1e-9; accepted at <= 1e-6 like every fit).
                                  attr_poly_far_set[type] = index of the type's far set in attr_poly_typed_pk, or -1; the kernel's
                                  LDS limits poly_num_slots + attr_poly_far_slots to 9 (the host gives the 2-/3-hop types and the
                                  single bonds their far sets first) */
  const int32_t* attr_poly_far_set; /* [100] or null */
  float attr_poly_far_hi;      /* upper end of that range (agdiff_amd/packing.py: 10 x cutoff); longer edges keep the encoder MLP */
  int64_t tune_cfconv_four_min_quads; /* [8192] agdiff_cfconv_node at poly_kt 1: from this many quads on (two per wave of 256 x 16),
                                         16-wave workgroups at 128 VGPRs = four waves per SIMD, groups of two channel tiles;
                                         below, the 12-wave shape (more workgroups for the same quads); -1: never */
  int32_t dist_union_kinks;    /* K: kink slots at the head of dist_union (a power of two in [2, 512]) */
  int32_t dist_union_segments; /* S: segments (= kinks in (0, cutoff] + 1 <= K) whose lines follow */
  /* The LOCAL head's edge_attr half by polynomial (agdiff_local_head): layers.0.weight[:, 128:] @ edge_attr(d, type) of
   * grad_local_dist_mlp is linear in the edge_attr row, and the row of a slotted type is a 32-term polynomial of d, so the
   * product is one too -- one k-tile per edge instead of four, and no 512-byte row to read.  One coefficient set per local
   * edge type whose fit the host accepted (packing.py fit_head_local: <= POLY_TOL like every fit), packed in precision_local
   * with head_local's first-layer scale; only with poly_kt == 1. */
  const float* head_local_poly_pk;     /* [head_local_near_sets + head_local_far_sets] x pkk [1][8] or null: the near sets (d in
                                          [0, cutoff]) in order of expected row count, then the far sets (d in (cutoff,
                                          attr_poly_far_hi]); the first tune_local_head_lds_sets stay in LDS, the others are read
                                          from L2 by the tiles that meet them */
  const int32_t* head_local_near_set;  /* [100] or null: edge type -> index of its near set in head_local_poly_pk, or -1 */
  const int32_t* head_local_far_set;   /* [100] or null: ... of its far set, or -1 (its rows beyond the cutoff read l_attr_rows) */
  int32_t head_local_near_sets;
  int32_t head_local_far_sets;
  int32_t tune_local_head_poly_off;    /* [0] 1: the local head reads the edge_attr rows for every tile (k_pair_head) */
  int32_t tune_local_head_lds_sets;    /* [0 = 4] coefficient sets of the local head kept in LDS next to its weights (at most 4:
                                          96 KiB of weights + 4 x 16 KiB); -1: none, every set is read from L2 */
} agdiff_params_t;

/* bits of agdiff_ws_t.variant_log: which kernel variants the launchers chose since the host last cleared it */
#define AGDIFF_VAR_CFCONV_NODE 1        /* agdiff_cfconv_node: radius rows (+ local quad tiles) by filter polynomials */
#define AGDIFF_VAR_CFCONV_NODE_LOCAL 2  /* ... its local quad tiles ran (every local type has a polynomial) */
#define AGDIFF_VAR_CFCONV_LOCAL_MLP 4   /* agdiff_cfconv_local: local edges through the filter MLPs */
#define AGDIFF_VAR_CFCONV_FUSED 8       /* agdiff_cfconv_fused: every edge through the filter MLPs */
#define AGDIFF_VAR_NODE_LDSW 16         /* node stage with workgroup-shared LDS weights */
#define AGDIFF_VAR_NODE_STREAM 32       /* node stage, one wave per tile streaming from L2 */
#define AGDIFF_VAR_NODE_SPLIT4 64       /* node stage, four waves per tile */
#define AGDIFF_VAR_GIN_LDSW 128         /* GIN layer with workgroup-shared LDS weights */
#define AGDIFF_VAR_SHARE_ROWS 256       /* local edge_attr rows written by the global encoder pass */
#define AGDIFF_VAR_ATTR_POLY 512        /* local edge_attr rows from per-type polynomials (agdiff_local_edge_rows) */
#define AGDIFF_VAR_HEAD_POLY 1024       /* global head with the edge_attr half from the d-polynomial */
#define AGDIFF_VAR_SIDE_STREAM 2048     /* local branch forked onto the side stream */
#define AGDIFF_VAR_POLY_L2_SETS 4096    /* agdiff_cfconv_node: some local types' coefficient sets did not fit in LDS (read from L2) */
#define AGDIFF_VAR_FUSED_FRONT 8192     /* agdiff_sampler_front: update of step t + radius graph of step t + 1 in one launch */
#define AGDIFF_VAR_CFCONV_NODE_FOUR 16384 /* agdiff_cfconv_node ran its four-waves-per-SIMD shape (tune_cfconv_four_min_quads) */
#define AGDIFF_VAR_CFCONV_NODE_QUAD 32768 /* agdiff_cfconv_node walked the radius rows in quad tiles (tune_cfconv_quad_tiles) */
#define AGDIFF_VAR_LOCAL_HEAD_POLY 131072 /* agdiff_local_head: the local head took the edge_attr half of its first layer from per-type
                                           polynomials over the type-pure tiles (topo->lh_*) */
#define AGDIFF_VAR_GRAPH_LARGE 65536    /* graph build without adjacency masks (agdiff_graph_build_large: a molecule of more than
                                           AGDIFF_MAX_ATOMS_PER_GRAPH atoms in the batch, or called directly) */

/* ---- static topology of one packed batch (host builds it once per batch) ---------------------
 * Graphs are contiguous node ranges (PyG Batch, utils/misc.py:88-90).  "Local" edges are the
 * bond / 2-hop / 3-hop edges (type > 0, dualenc.py:566); they never depend on positions. */
typedef struct agdiff_topo {
  int64_t num_nodes;         /* N */
  int64_t num_graphs;        /* G */
  int64_t num_local;         /* L: local edges, in reference order (sorted by (src, dst)) */
  int64_t max_edges;         /* capacity of the per-edge buffers: sum_i (33 + local in-degree_i) */
  int64_t max_atoms_per_graph; /* <= AGDIFF_MAX_ATOMS_LARGE; above AGDIFF_MAX_ATOMS_PER_GRAPH the graph builds take the large path and
                                agdiff_sampler_front refuses (AGDIFF_ERR_LIMIT) */
  int64_t max_in_degree;     /* max_i (33 + local in-degree_i); any value (a list may span several chunks) */
  const int32_t* graph_ptr;  /* [G+1] node offsets */
  const int32_t* atom_type;  /* [N] */
  const int32_t* loc_src;    /* [L] */
  const int32_t* loc_dst;    /* [L] */
  const int32_t* loc_type;   /* [L] (1..99) */
  const int32_t* loc_out_ptr;/* [N+1]: local edges with src == i are [loc_out_ptr[i], loc_out_ptr[i+1]) */
  const int32_t* loc_in_ptr; /* [N+1] */
  const int32_t* loc_in_eid; /* [L]: local edge ids grouped by dst (src ascending) */
  /* canonical local edges: the local edges j -> i and i -> j carry the same type and length, hence the same edge_attr and
   * the same local-head output (h_i * h_j is symmetric); one of the two (src < dst) is canonical, as is every local edge
   * without such a mirror.  Static like the local list itself. */
  int64_t num_local_canon;   /* Lc */
  const int32_t* lc_src;     /* [Lc] */
  const int32_t* lc_dst;     /* [Lc] */
  const int32_t* lc_type;    /* [Lc] */
  const int32_t* lc_pos;     /* [Lc]: the canonical edge's own id in the local list */
  const int32_t* lc_mir;     /* [Lc]: its mirror's id there, or -1 */
  const int32_t* loc_row;    /* [L]: canonical index (row of l_attr_rows) of every local edge */
  const int32_t* loc_in_src; /* [L]: loc_src[loc_in_eid[s]] (the GIN gather reads its indices by in-slot, one level deep) */
  const int32_t* loc_in_row; /* [L]: loc_row[loc_in_eid[s]] */
  /* the local list as a destination-sorted edge list of its own for the split CFConv, every non-empty target's list PADDED to
   * at least 8 entries: a 16-edge tile then holds at most three targets with the middle one's list whole, which the
   * kernels' fast reduction covers (local in-degrees are ~8: unpadded, many tiles would hold four or more and take the
   * general reduction).  Pad entries: src = dst = the target, type of the list's first edge, and nothing ever writes their
   * CFConv scale (zero-initialised): they contribute exactly 0. */
  int64_t num_local_padded;  /* Lp */
  const int32_t* lp_ptr;     /* [N+1]: padded list of target i = [lp_ptr[i], lp_ptr[i+1]) */
  const int32_t* lp_src;     /* [Lp] */
  const int32_t* lp_dst;     /* [Lp] */
  const int32_t* lp_type;    /* [Lp] */
  const int32_t* lp_row;     /* [Lp]: canonical index (row of l_attr_rows) of the entry's edge, -1 for pad entries */
  const int32_t* lc_ppos;    /* [Lc]: padded-list position of the canonical edge */
  const int32_t* lc_pmir;    /* [Lc]: ... of its mirror, or -1 */
  /* QUADS of targets for agdiff_cfconv_node: one wave owns the four targets quad_tgt[4 p .. 4 p + 3] of ONE molecule (-1: none,
   * in the last quad of a molecule).  The local edges once more as quad tiles: a 16-row tile holds rows of ONE edge type;
   * rows 4 k .. 4 k + 3 are in-edges of that type of the quad's k-th target (in order of source; a target with more than
   * four gets another tile of the type), pad rows: src = the target itself, the tile's type, and nothing ever writes their
   * CFConv scale: they contribute exactly 0.  The four rows one lane quarter holds then belong to ONE target, so the sum
   * over a target's edges needs no masks, and a tile needs ONE filter set.  The host groups atoms whose in-lists need like
   * numbers of tiles per type; tiles of quad p: type ascending */
  int64_t num_quads;         /* Q */
  int64_t group_targets;     /* GT = 4, 2 or 1: targets per quad that are used (small batches: fewer targets per wave, more waves).
                                A tile then gives each target 16 / GT rows: rows (16 / GT) k .. of the k-th target; entries
                                quad_tgt[4 p + GT ..] are -1 */
  const int32_t* quad_tgt;   /* [4 Q] */
  const int32_t* lcm_ptr;    /* [G+1]: the canonical local edges lc_*[lcm_ptr[g] .. lcm_ptr[g+1]) belong to molecule g (the list is
                                sorted by molecule, then edge type, then source) */
  int64_t local_type_mask[2];/* bit t of the 128-bit mask: the batch has a local edge of type t */
  int64_t num_local_tiles;   /* T = lt_ptr[Q] */
  const int32_t* lt_ptr;     /* [Q + 1]: tiles of quad p are [lt_ptr[p], lt_ptr[p+1]) */
  const int32_t* lt_src;     /* [16 T] */
  const int32_t* lt_type;    /* [16 T] (the same for the 16 rows of a tile) */
  const int32_t* lc_tpos;    /* [Lc]: quad-tile row of the canonical edge */
  const int32_t* lc_tmir;    /* [Lc]: ... of its mirror, or -1 */
  const int32_t* quad_wg_ptr;/* [257] or null: workgroup w of agdiff_cfconv_node's 256 persistent workgroups (k_cfconv_quad) owns the quads
                                [quad_wg_ptr[w], quad_wg_ptr[w+1]) -- contiguous ranges of like tile counts; null (or fewer workgroups):
                                equal quad counts */
  /* The canonical local edges once more for the local head (agdiff_local_head): a static permutation whose 16-row tiles each hold
   * ONE edge type.  The canonical list is cut into runs of consecutive molecules (the shortest power of two for which the pad
   * rows stay under 8 % of the rows); inside a run the edges are sorted by type, and every (run, type) segment is padded to a
   * multiple of 16 rows -- a molecule's h rows stay in one L2, and a tile needs one coefficient set.  Only the head walks it. */
  int64_t num_head_tiles;    /* Th */
  const int32_t* lh_idx;     /* [16 Th]: canonical index (row of l_attr_rows, entry of lc_len) of the row's edge, -1 for pad rows */
  const int32_t* lh_src;     /* [16 Th]: lc_src / lc_dst / lc_pos / lc_mir of that edge (pad rows: 0, 0, -1, -1) */
  const int32_t* lh_dst;
  const int32_t* lh_pos;
  const int32_t* lh_mir;
  const int32_t* lh_type;    /* [Th]: the tile's edge type */
  const int32_t* loc_bits;   /* (null for batches with max_atoms_per_graph > AGDIFF_MAX_ATOMS_PER_GRAPH) [N][W], W = 2 ceil(max_atoms_per_graph / 64) 32-bit words, or null: the static local in-adjacency of
                                every atom as a bit mask over its molecule's atoms -- bit (j - graph_ptr[g]) of row i is set when
                                the local edge j -> i exists.  agdiff_sampler_front copies a molecule's rows into LDS (the radius
                                graph excludes local pairs); null: it builds them from loc_in_ptr / loc_in_eid / loc_src per step */
} agdiff_topo_t;

/* ---- workspace (device buffers the host allocates once per batch) ------------------------- */
typedef struct agdiff_ws {
  /* dynamic graph, destination-sorted: edges of target i are [in_ptr[i], in_ptr[i+1]) with src ascending */
  int32_t* num_edges;        /* [1]  E (device scalar, rewritten by every graph build) */
  int32_t* num_local;        /* [1]  L as a device scalar (written once by the host) */
  int32_t* graph_edge_cnt;   /* [G]  */
  int32_t* graph_edge_ptr;   /* [G+1] */
  int32_t* in_ptr;           /* [N+1] */
  int32_t* out_ptr;          /* [N+1]: reference order (sorted by (src,dst)): edges with src == i */
  int32_t* e_src;            /* [max_edges] */
  int32_t* e_dst;            /* [max_edges] */
  int32_t* e_type;           /* [max_edges] */
  float*   e_len;            /* [max_edges] */
  int32_t* ref2dst;          /* [max_edges]: reference position q -> destination-sorted id */
  int32_t* e_loc;            /* [max_edges]: row of l_attr_rows (= canonical index, topo->loc_row) of the edge's local (type > 0)
                                list entry, -1 for radius-only edges */
  /* canonical edges: j -> i and i -> j with equal type have the same length and type, hence bit-identical
   * edge_attr and pair-head output (dualenc.py:189-211); one of the two (src < dst) is canonical, as is every edge
   * without such a mirror.  Destination-sorted like the full list; the encoder and the global head walk this list. */
  int32_t* num_canon;        /* [1]  device scalar */
  int32_t* graph_canon_cnt;  /* [G]  */
  int32_t* graph_canon_ptr;  /* [G+1] */
  float*   c_len;            /* [max_edges] */
  int32_t* c_type;           /* [max_edges] */
  int32_t* c_src;            /* [max_edges] */
  int32_t* c_dst;            /* [max_edges] */
  int32_t* c_pos;            /* [max_edges]: the canonical edge's own id in the destination-sorted list */
  int32_t* c_mir;            /* [max_edges]: its mirror's id there, or -1 */
  float*   e_attr;           /* [ceil(max_edges/16)] tiles x 2048 floats: edge_attr in operand form (csrc/common.hpp) */
  float*   e_inv_global;     /* [max_edges] grad_global_dist_mlp output, destination-sorted */
  float*   e_scale;          /* [2*num_convs][ceil(max_edges/16)*16]: lw(d)*C(d) of conv1 / conv2 of every block (schnet.py:138-149) */
  /* local edges (reference order) */
  float*   l_len;            /* [L] */
  float*   lc_len;           /* [Lc] lengths of the canonical local edges (same values as l_len[lc_pos]) */
  int32_t* num_local_canon;  /* [1]  Lc as a device scalar (written once by the host) */
  float*   l_attr_rows;      /* fp32 row-major edge_attr rows [128] of the local edges (GIN message gather, local head): ONE row
                                per canonical local edge (row c for lc_*[c]; a mirror pair shares it: the GIN layers are
                                bound by reading these rows), written by the global encoder pass through e_loc when that
                                pass runs, else by a pass over the canonical local list.  With a caller-supplied graph
                                (AGDIFF_FWD_GRAPH_GIVEN: lengths need not be symmetric) one row per local edge [L]. */
  float*   l_inv;            /* [L] grad_local_dist_mlp output */
  /* nodes */
  float*   h;                /* [N][128] SchNet node state */
  float*   xs;               /* [N][192] lin1/BN/LeakyReLU outputs feeding conv1 (0..127) and conv2 (128..191) */
  float*   agg;              /* [N][192] CFConv aggregates */
  float*   agg_first;        /* [chunks][192], chunks = ceil(ceil(max_edges/16) / agdiff_conv_chunk_tiles(max_edges)) (agdiff_cfconv_fused):
                                partial sum of the target whose list was already open when the chunk started; the node stage
                                adds them in chunk order */
  float*   hl;               /* [N][128] GIN node state (ping) */
  float*   hl2;              /* [N][128] (pong) */
  int32_t* nan_flag;         /* [1 + G]: [0] set to 1 when any position becomes NaN, [1 + g] when one of graph g does
                                (sticky: the host clears them when a sampling job starts) */
  int32_t* range_rows;       /* [N] or null.  Split-fp16 operands saturate at 65504: the kernels that convert activations which
                                depend on the STATE and which no tensor of the workspace shows (hidden layers of the node stage, the
                                GIN layers, the pair heads) set range_rows[node] = 1 when such a value of that node (of an edge's
                                source node) reaches 65000 -- and, where they store them, when a node state (|h|, |hl| >= 255: the
                                heads multiply two) or a CFConv input (|xs| >= 60000) leaves the range the host's tensor watch
                                polls, so that an excursion between two polls is not lost.  The node's results are then not to be
                                trusted in this mode: the caller
                                polls the flags with the NaN flag, clears them and runs the owning molecules in split-bf16
                                (agdiff_amd/epsnet.py range_report).  Never written in the other modes. */
  /* CFConv by filter polynomials (agdiff_params_t.poly_kt > 0): the radius edges (type 0) of the dynamic graph by TARGET, in
   * AGDIFF_RAD_STRIDE rows per target (written by agdiff_graph_build next to the full list; sources ascending).  Rows
   * [rad_cnt[i], 16 ceil(rad_cnt[i] / 16)) of target i are pad rows (src = i, length 0, scale 0: agdiff_edge_scales_split
   * writes them), rows beyond are never read by k_cfconv_node: every 16-row tile belongs to ONE target.  On quads
   * (topo->group_targets == 4, p->tune_cfconv_quad_tiles >= 0: k_cfconv_quad) agdiff_sampler_front does NOT write the pad rows:
   * that kernel runs rows [rad_cnt[i], 4 ceil(max over the quad / 4)) with scale 0 itself and only needs them to hold valid
   * indices and finite numbers -- older rows of the same molecule, or the zeros the host allocated the buffers with. */
  int32_t* rad_cnt;          /* [N]  radius edges of target i (<= AGDIFF_RADIUS_CAP) */
  int32_t* rad_src;          /* [N * AGDIFF_RAD_STRIDE] */
  float*   rad_len;          /* [N * AGDIFF_RAD_STRIDE] */
  float*   r_scale;          /* [2*num_convs][N * AGDIFF_RAD_STRIDE]: lw(d)*C(d) by radius-list row */
  int32_t* num_local_padded; /* [1]  Lp as a device scalar (written once by the host) */
  float*   l_scale;          /* [2*num_convs][ceil(Lp/16)*16]: the same by padded-list position (pad entries stay 0) */
  float*   l_attr_frag;      /* [ceil(Lp/16)] tiles x 2048 floats: edge_attr of the local edges in operand form, by padded-list
                                position (only written / read when the local edges go through the filter MLPs) */
  float*   l_len_p;          /* [Lp] lengths of the local edges by padded-list position (agdiff_local_lengths; pads stay 0) */
  int32_t* g_inbits;         /* (may be null; never used by agdiff_graph_build_large) [N][2 * ceil(max_atoms_per_graph / 64)] hand-over from the graph build's count pass to its fill
                                pass: row i = in-adjacency bit mask of atom i inside its molecule (optional, with g_deg / g_cdeg) */
  int32_t* g_deg;            /* [N] in-degrees (agdiff_graph_build_large, which needs both: each target's candidate threshold) */
  int32_t* g_cdeg;           /* [N] canonical in-degrees (agdiff_graph_build_large: then their exclusive scan) */
  int32_t* enc_flags;        /* [1 + ceil(Lc/16)]: agdiff_local_edge_rows: [0] = tiles of the canonical local list that hold an edge
                                longer than the cutoff (or of a type without a polynomial) this step, [1 + tile] = the 16-bit mask
                                of those rows: the encoder MLP evaluates exactly them, the polynomials all the others */
  float*   h0;               /* [N][128] cache of node stage 0's h (the atom embeddings: they do not depend on the positions) */
  float*   xs0;              /* [N][192] ... and of its xs (block 0's lin1 / BN / LeakyReLU outputs) */
  float*   agg_loc;          /* [N][192] CFConv aggregates over the local edges (agdiff_cfconv_local) */
  float*   agg_first_loc;    /* [ceil(ceil(Lp/16) / agdiff_conv_chunk_tiles(Lp))][192] */
  float*   lt_len;           /* [16 T] lengths of the local edges by quad-tile row (agdiff_local_lengths; pads stay 0) */
  float*   lt_scale;         /* [2*num_convs][16 T]: lw(d)*C(d) by quad-tile row (pad rows stay 0) */
  float*   inv_r;            /* [N * AGDIFF_RAD_STRIDE] grad_global_dist_mlp output by radius row (fused sampler front) */
  int32_t* canon_counter;    /* [2] live length of the fused sampler front's canonical radius list, by step parity: every molecule
                                claims its range of ws->c_* with one atomic add on [parity] (and molecule 0 zeroes the other) */
  int64_t* variant_log;      /* [host] one word or null: every launcher ORs the AGDIFF_VAR_* bit of the variant it chose */
} agdiff_ws_t;

typedef struct agdiff_step_args {
  const float* pos_in;       /* [N][3] */
  float*       pos_out;      /* [N][3] (may alias pos_in) */
  float*       scratch;      /* [N][3] uncentred positions between the two passes of the update */
  const float* noise;        /* [N][3] standard normal draws for this step (torch.randn_like, dualenc.py:529) */
  float*       traj_out;     /* [N][3] or null: copy of the centred positions (pos_traj, dualenc.py:545) */
  float sigma;               /* sigmas[i] */
  float step_size;           /* step_lr * (sigmas[i] / 0.01) ** 2, evaluated by the host in fp32 (dualenc.py:532) */
  float noise_scale;         /* sqrt(step_size * 2) (dualenc.py:536) */
  float w_global;
  float clip;                /* clip_norm limit of the global term (dualenc.py:522) */
  float clip_local;          /* < 0: no local clipping (clip_local=None) */
  float clip_pos;            /* < 0: no clamp */
  int32_t use_global;        /* sigmas[i] < global_start_sigma (dualenc.py:515) */
} agdiff_step_args_t;

/* Tiles per chunk the fused CFConv kernel and the node stage use for a workspace of `max_edges` edges (1..8):
 * small batches get short chunks so that every wave slot of the chip has work. */
int agdiff_conv_chunk_tiles(int64_t max_edges);

/* Host helper of the topology builder (no GPU work): the order of a molecule's n atoms in which consecutive runs of `gt`
 * atoms form the target groups agdiff_cfconv_node's waves own (agdiff_topo_t.quad_tgt).  need [n][k] (row-major): local
 * 16-row tiles atom i needs of local edge type k = ceil(in-edges of that type / (16 / gt)); a group costs the sum over the
 * types of the MAX of its atoms' needs, so atoms with like needs belong together.  Search: the atoms sorted by their need
 * vectors with each type in turn as the leading key, or by total need; from every start, swaps of two atoms between two
 * groups while the total falls; the cheapest result wins (ties: the earliest start).  Deterministic.  order_out [n]. */
int agdiff_group_order(const int32_t* need /* [host] */, int32_t n, int32_t k, int32_t gt, int32_t* order_out /* [host] */);

/* Build stamp / ABI check. */
int agdiff_abi_version(void);
/* sizeof() of every struct above, for the binding's self-check: out[0..6] =
 * conv, gin, head, params, topo, ws, step_args. */
int agdiff_struct_sizes(int64_t* out /* [host] */);

/* torch_cluster.radius_graph + sparse add/coalesce (models/common.py:208-233) + get_distance
 * (geometry.py:5-6): rebuilds the destination-sorted edge list, its reference-order permutation,
 * edge types and lengths from `pos`. */
int agdiff_graph_build(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff, void* stream);
/* The same with canon_radius_only != 0: the canonical list (ws->c_*, num_canon) holds RADIUS edges only -- one of j -> i /
 * i -> j when both are radius edges.  What the denoising loop asks for (AGDIFF_FWD_SAMPLER with poly_kt > 0): there only
 * the global head walks the canonical list, and only radius edges' results are used. */
int agdiff_graph_build_ex(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff,
                          int32_t canon_radius_only, void* stream);

/* The same with the radius rows' CFConv scales (ws->r_scale, all 2 * num_convs of them: DistanceWeightingNetwork x cutoff
 * envelope, encoder/schnet.py:83-100,138-149) and the pad rows of every target's last tile written by the fill pass itself:
 * what the denoising loop calls (one launch less per step than agdiff_graph_build_ex + agdiff_edge_scales_split(0)). */
int agdiff_graph_build_scaled(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos,
                              float cutoff, int32_t canon_radius_only, void* stream);

/* The same graph, bit for bit and in the same order, built WITHOUT per-molecule adjacency masks (csrc/graph.hip, k_lg_*): for
 * molecules of up to AGDIFF_MAX_ATOMS_LARGE atoms, a molecule spread over ceil(n / 16) workgroups.  The three entry points above
 * take this path by themselves when topo->max_atoms_per_graph > AGDIFF_MAX_ATOMS_PER_GRAPH; called directly it serves any batch.
 * p null: as agdiff_graph_build_ex; p given: as agdiff_graph_build_scaled.  Needs ws->g_deg and ws->g_cdeg (scratch); reads neither
 * ws->g_inbits nor topo->loc_bits.  Five launches; deterministic (offsets from scans over the atoms, no atomics). */
int agdiff_graph_build_large(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos,
                             float cutoff, int32_t canon_radius_only, void* stream);
/* Launch shape of agdiff_graph_build_large for this batch: out[0] = workgroups per launch, out[1] = atoms (targets) per workgroup. */
int agdiff_graph_large_grid(const agdiff_topo_t* topo, int64_t* out /* [host] */);

/* get_distance on the static local edges (geometry.py:5-6 applied to edge_index[:, local_edge_mask]): one evaluation per
 * canonical local edge, written to l_len of the edge and of its mirror, to lc_len and -- where the workspace has them --
 * to l_len_p (padded-list positions) and lt_len (quad-tile rows). */
int agdiff_local_lengths(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, void* stream);

/* DistanceWeightingNetwork x cutoff envelope of all 2*num_convs CFConvs (encoder/schnet.py:83-100, 138-149):
 * ws->e_scale from ws->e_len; per_canonical_edge != 0: from ws->c_len, one evaluation per canonical edge written to its
 * position and its mirror's (equal lengths: the same value bit for bit). */
int agdiff_edge_scales(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                       int32_t per_canonical_edge, void* stream);

/* get_edge_encoder(cfg)(edge_length, edge_type) (encoder/edge.py:106-116): MLPEdgeEncoder.forward
 * (edge.py:84-103) when p->edge_encoder == 0, GaussianSmearingEdgeEncoder.forward (edge.py:34-42) when 1.
 * n_edges_dev: device scalar with the live edge count (<= max_tiles*16).  Outputs, each optional:
 *   attr_frag  operand-form edge_attr tiles;
 *   attr_rows  fp32 rows [.][128]: row e of edge e, or row row_index[e] when row_index is given (negative: no
 *              row) -- how the pass over all edges also serves the local edge list.
 * pos_index / mir_index (both or neither): the n edges are a canonical list (agdiff_ws_t.c_*); edge e's results go
 * to position pos_index[e] and, when >= 0, mir_index[e] of attr_frag / row_index instead of position e. */
int agdiff_edge_encoder(const agdiff_params_t* p, const int32_t* n_edges_dev, int64_t max_tiles,
                        const float* e_len, const int32_t* e_type, float* attr_frag, float* attr_rows,
                        const int32_t* row_index, const int32_t* pos_index, const int32_t* mir_index, void* stream);

/* edge_attr rows of the canonical local edges (ws->l_attr_rows, one row per canonical edge: what the GIN layers and the
 * local head read; dualenc.py:214-216): with per-type polynomials available (p->attr_poly_typed_pk, p->poly_num_slots > 0)
 * every 16-edge tile whose lengths all lie inside [0, cutoff] takes its rows from them; a tile with a longer edge (bonded
 * atoms far apart at high sigma) is flagged and goes through agdiff_edge_encoder's MLP.  Without polynomials: the MLP for
 * all of them.  Needs ws->lc_len (agdiff_local_lengths). */
int agdiff_local_edge_rows(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, void* stream);

/* Node-side stage k of SchNetEncoder.forward (encoder/schnet.py:268-282): k == 0 embeds atoms;
 * k >= 1 finishes InteractionBlock k-1 (lin2/BN, act, lin, gate, AdaptiveScaling, residual);
 * k < num_convs also applies block k's conv{1,2}.lin1/BN/LeakyReLU into ws->xs.  Block k-1's aggregates are ws->agg /
 * ws->agg_first by chunks of the full edge list (agdiff_cfconv_fused). */
int agdiff_schnet_node_stage(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t k, void* stream);
/* The same with `split` bits: 1: block k-1's aggregates are ws->agg as agdiff_cfconv_node wrote it (one complete row per
 * node); 8 (with 1): plus ws->agg_loc / ws->agg_first_loc of agdiff_cfconv_local (lists topo->lp_ptr).  4 (k == 0): write
 * the stage's h / xs to the cache ws->h0 / ws->xs0; 2 (k == 1): block 0's input h is ws->h0. */
int agdiff_schnet_node_stage_split(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t k,
                                   int32_t split, void* stream);

/* CFConv filter generation + message + aggr='add' for both convs of block k
 * (encoder/schnet.py:138-162; PyG MessagePassing.propagate): ws->agg / ws->agg_first. */
int agdiff_cfconv_fused(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t k, void* stream);

/* The same two CFConvs with the filters from d-polynomials (agdiff_params_t.poly_kt > 0), one launch, one wave per QUAD of
 * targets: the radius rows of each (ws->rad_*, ws->r_scale; p->conv[k].filt_poly_pk) and -- when agdiff_local_poly_enabled
 * -- the quad's local tiles (topo->lt_*, ws->lt_len, ws->lt_scale; per-type sets p->conv[k].filt_poly_typed_pk) are
 * summed in registers and ws->agg[i] is written once, complete, for every node (zeros for a node without edges).  Without
 * local polynomials the local edges' part comes from agdiff_cfconv_local: the filter MLPs over the padded local list
 * (topo->lp_*, ws->l_scale, ws->l_attr_frag) -> ws->agg_loc / ws->agg_first_loc, added by the node stage (split bit 8).
 * agdiff_edge_scales_split fills ws->r_scale and the radius pad rows (which == 0), ws->l_scale (1) or ws->lt_scale (2). */
int agdiff_cfconv_node(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t k, void* stream);
int agdiff_cfconv_local(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t k, void* stream);
/* How the local edges' CFConv filters are evaluated for this (model, batch):
 *   1  all by per-type d-polynomials inside agdiff_cfconv_node (every local type of the batch has a slot; topo->lt_*,
 *      ws->lt_len, ws->lt_scale present; not switched off by p->tune_local_poly_off);
 *   2  mixed: the slotted types as in 1, the others by agdiff_cfconv_local (filter MLPs on ws->l_attr_frag, where
 *      agdiff_edge_scales_split(which = 1) leaves the slotted types' scales at 0);
 *   0  all by agdiff_cfconv_local. */
int agdiff_local_poly_enabled(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws);
int agdiff_edge_scales_split(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t which,
                             void* stream);

/* agdiff_pair_head with p->head_global for edges whose edge_attr is MLPEdgeEncoder(len, type 0): the edge_attr half of the
 * first layer comes from the d-polynomial head_global.attr_poly_pk (needs p->poly_kt > 0).  pos_index / mir_index as in
 * agdiff_pair_head (both or neither). */
int agdiff_pair_head_poly(const agdiff_params_t* p, const int32_t* n_edges_dev, int64_t max_tiles,
                          const int32_t* src, const int32_t* dst, const float* len, const float* node_h,
                          const int32_t* pos_index, const int32_t* mir_index, float* out, void* stream);

/* assemble_atom_pair_feature + grad_*_dist_mlp (models/common.py:106-109, 86-103; dualenc.py:203-211,
 * 226-239) over n edges given by (src, dst); edge_attr either as operand-form tiles (attr_frag) or as fp32
 * rows [n][128] (attr_rows) -- exactly one of the two.  pos_index / mir_index (both or neither, with attr_frag):
 * the n edges are a canonical list; edge e reads its attrs at position pos_index[e] and writes its result to
 * out[pos_index[e]] and, when >= 0, out[mir_index[e]] (h_i * h_j is symmetric, so the mirror's value is the same).
 * With attr_rows the edge's attributes are row e of attr_rows, whatever pos_index is (the local head over the canonical
 * local list: row c, results to out[lc_pos[c]] and out[lc_mir[c]]). */
int agdiff_pair_head(const agdiff_head_params_t* hp, const int32_t* n_edges_dev, int64_t max_tiles,
                     const int32_t* src, const int32_t* dst, const float* node_h, const float* attr_frag,
                     const float* attr_rows, const int32_t* pos_index, const int32_t* mir_index, float* out,
                     void* stream);

/* GINEncoder.forward (encoder/gin.py:112-148) on the static local edges; result in ws->hl.
 * rows_per_canonical_edge != 0: ws->l_attr_rows holds one row per canonical local edge (local edge e reads row
 * topo->loc_row[e]); 0: one row per local edge. */
int agdiff_gin_encoder(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                       int32_t rows_per_canonical_edge, void* stream);

/* PyG MessagePassing.propagate(aggr='add') with message x_j * W (encoder/schnet.py:156,161-162) as a
 * stand-alone op on a destination-sorted CSR: out[i][:] = sum_{e in [in_ptr[i], in_ptr[i+1])} x[src[e]][:] * W[e][:].
 * F must be 64 or 128. */
int agdiff_cfconv_aggregate(const float* x, const float* W, const int32_t* in_ptr, const int32_t* src,
                            int64_t num_nodes, int32_t F, float* out, void* stream);

/* The whole score network, dualenc.py:142-251.  flags:
 *   AGDIFF_FWD_GLOBAL       run the global branch; without it everything whose result the sampler discards
 *                           when sigma >= global_start_sigma (dualenc.py:523-524) is skipped
 *   AGDIFF_FWD_NO_RADIUS    extend_radius=False (dualenc.py:166-176): the graph is the bond graph only
 *   AGDIFF_FWD_GRAPH_GIVEN  caller-supplied edge_index / edge_type / edge_length (dualenc.py:165): ws already
 *                           holds the destination-sorted graph (num_edges, in_ptr, e_src/e_dst/e_type/e_len)
 *                           and l_len; neither is rebuilt from `pos` */
#define AGDIFF_FWD_GLOBAL 1
#define AGDIFF_FWD_NO_RADIUS 2
#define AGDIFF_FWD_GRAPH_GIVEN 4
/*   AGDIFF_FWD_SAMPLER      the caller is the denoising loop: of the global head's outputs only those of radius edges are
 *                           used (edge_inv_global * (1 - local_edge_mask), dualenc.py:516-518), so with
 *                           poly_kt > 0 neither the edge encoder nor the head runs on anything but d-polynomials and the
 *                           local list; ws->e_inv_global is then only valid at radius edges */
#define AGDIFF_FWD_SAMPLER 8
/*   AGDIFF_FWD_STAGE0_CACHED ws->h0 / ws->xs0 already hold node stage 0's outputs for this topology and these weights (an
 *                           earlier call with AGDIFF_FWD_GLOBAL on the same workspace wrote them): stage 0 -- embedding
 *                           look-up and block 0's lin1, which do not depend on `pos` -- is not launched again */
#define AGDIFF_FWD_STAGE0_CACHED 16
/*   AGDIFF_FWD_GRAPH_READY  (with AGDIFF_FWD_SAMPLER, poly_kt > 0) agdiff_sampler_front has already built this step's radius rows,
 *                           their scales and its canonical radius list from `pos` (and written the local edges' lengths and
 *                           quad-tile scales): no graph build here; the global head's outputs go to ws->inv_r (by radius
 *                           row), where the next agdiff_sampler_front reads them.  AGDIFF_FWD_PARITY: the step's parity bit
 *                           (which of ws->canon_counter[2] holds the list's length) */
#define AGDIFF_FWD_GRAPH_READY 32
#define AGDIFF_FWD_PARITY 64
/*   AGDIFF_FWD_GRAPH_PENDING (with AGDIFF_FWD_GRAPH_READY) the front has run its update and local phases only (mode 1 | 4): the
 *                           graph phase (mode 2) is launched here, on `stream`, AFTER the local branch has been forked onto the
 *                           side stream -- the local branch then runs beside it instead of beside the first CFConv */
#define AGDIFF_FWD_GRAPH_PENDING 128
int agdiff_score_forward(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                         const float* pos, int32_t flags, void* stream);

/* The serial front of a denoising step in ONE launch (csrc/front.hip), one workgroup per molecule:
 *   mode & 1  the Langevin update of the step described by `s` (eq_transform x 2, clip_norm, move, NaN check, center_pos,
 *             clamp, trajectory row: geometry.py:9-17, dualenc.py:506-545, 581-589) from ws->l_inv and -- when
 *             s->use_global -- ws->inv_r over the radius rows the last graph phase wrote;
 *   mode & 2  then the radius graph of the NEXT forward on the positions just written (s->pos_out; s->pos_in without an
 *             update): ws->rad_cnt / rad_src / rad_len / r_scale with pad rows, and the canonical radius list ws->c_len /
 *             c_src / c_dst / c_pos / c_mir (c_pos / c_mir = radius rows) of live length ws->canon_counter[parity], parity =
 *             (mode >> 4) & 1 alternating from step to step.  `cutoff` = p->cutoff, or 0 for extend_radius = False;
 *   mode & 4  and, on the same positions, what agdiff_local_lengths and agdiff_edge_scales_split(which = 2) write: the local
 *             edges' lengths in every layout (ws->l_len, lc_len, l_len_p, lt_len) and their CFConv scales by quad-tile row
 *             (ws->lt_scale) -- agdiff_score_forward then skips both (AGDIFF_FWD_GRAPH_READY).
 * The following agdiff_score_forward takes AGDIFF_FWD_SAMPLER | AGDIFF_FWD_GRAPH_READY.  Replaces agdiff_langevin_update +
 * agdiff_graph_build_scaled inside the denoising loop (models/common.py:208-233 is rebuilt every step). */
int agdiff_sampler_front(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                         const agdiff_step_args_t* s, int32_t mode, float cutoff, void* stream);
/* ONE denoising step of the loop above as a replayable HIP graph -- [agdiff_sampler_front(front_mode) | agdiff_score_forward(fwd_flags
 * on host_step->pos_in) | step counter + 1], captured from `stream` (side stream of the local branch included) and instantiated:
 * small batches (scripts/test.py:130-164 samples one molecule's 100..1000 conformers per call) are bound by the ~25 launches a step
 * takes, a replay is one call.  What changes from step to step does not sit in kernel arguments: the front kernel reads the
 * update's step from the DEVICE table `step_table` at index *step_index (the host fills the table for the whole run: noise and
 * trajectory rows, sigma, step size, ...), and the last node of the graph increments *step_index.  `host_step` only carries what
 * is the same for every step (pos_in / pos_out, and valid pointers for the argument checks).  One graph per (front_mode, fwd_flags)
 * the loop alternates between (step parity, global branch on / off).  The kernels must have run once outside a capture (their
 * function attributes, the side stream and its events are set up on first use).  *graph_out: opaque handle for
 * agdiff_step_graph_launch / agdiff_step_graph_destroy. */
int agdiff_step_graph_capture(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                              const agdiff_step_args_t* host_step /* [host] */, const agdiff_step_args_t* step_table,
                              int32_t* step_index, int32_t front_mode, float cutoff, int32_t fwd_flags, void* stream,
                              void** graph_out /* [host] */);
int agdiff_step_graph_launch(void* graph /* [host] */, void* stream);
int agdiff_step_graph_destroy(void* graph /* [host] */);

/* The polynomial global head (agdiff_pair_head_poly) over the canonical radius list of agdiff_sampler_front (step parity as
 * there): results to ws->inv_r at the entry's radius row and its mirror's. */
int agdiff_pair_head_poly_rows(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t parity,
                               void* stream);

/* grad_local_dist_mlp over the local edges (dualenc.py:226-239), what agdiff_score_forward's local branch ends with: ws->l_inv from
 * ws->hl and the edge_attr rows ws->l_attr_rows.  canonical != 0: one evaluation per canonical local edge, written to its own
 * and its mirror's entry of l_inv.  Then, when the host has packed head sets (agdiff_params_t.head_local_poly_pk), poly_kt == 1,
 * the encoder is the MLP one and tune_local_head_poly_off is 0, the head walks the type-pure tiles topo->lh_*: a tile whose
 * type has a set and whose lengths all lie in [0, cutoff] (or all in (cutoff, attr_poly_far_hi] with a far set) takes the
 * edge_attr half of the first layer from that set as ONE k-tile of ws->lc_len; every other tile -- a type without a set, a
 * length outside those ranges or not finite, both ranges in one tile -- reads its rows of l_attr_rows and runs the four
 * k-tiles with the arithmetic of agdiff_pair_head (bit-identical results for those tiles).  No atomics: reproducible. */
int agdiff_local_head(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, int32_t canonical, void* stream);

/* In-step timing of the dominant kernel (bench.py's roofline object): between agdiff_profile_cfconv(1) and (0) every CFConv
 * launch that agdiff_score_forward issues for the global branch (one InteractionBlock's agdiff_cfconv_node [+ agdiff_cfconv_local],
 * or agdiff_cfconv_fused) is bracketed by a pair of HIP events on the stream it runs on; agdiff_profile_cfconv_read waits for
 * them, returns their summed elapsed time and the number of bracketed launches, and resets the list.  [host] pointers. */
int agdiff_profile_cfconv(int32_t enable);
int agdiff_profile_cfconv_read(double* total_ms, int64_t* launches);

/* eq_transform x2, clip_norm, Langevin update, NaN check, center_pos, clamp
 * (geometry.py:9-17; dualenc.py:506-545, 581-589) from ws->l_inv / ws->e_inv_global. */
int agdiff_langevin_update(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const agdiff_step_args_t* a, void* stream);

/* Standard normals of the sampler -- noise = torch.randn_like(pos) of every denoising step (dualenc.py:529) and
 * pos_init = torch.randn(batch.num_nodes, 3) (scripts/test.py:146) -- from a COUNTER-BASED generator instead of a generator's
 * running state: out[s][a][0..2] is a pure function of (seed, stream_id[graph of atom a], index of a inside its graph, steps[s]),
 * so a conformer's draws do not depend on where it sits in the packed batch, on what is packed beside it or on how the batch is
 * cut over ranks.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key bumped by 0x9E3779B9 / 0xBB67AE85 per round) with
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (atom index inside its graph, steps[s], stream id low word, stream id high word);
 * steps[s] = the schedule index i of the step (the diffusion timestep the loop visits, not its loop counter), -1
 * (= 0xFFFFFFFF) is reserved for the initial positions.  A 32-bit output x gives u = ((x >> 8) + 0.5) 2^-24 in (0, 1); with
 * r(u) = sqrt(-2 ln u): out[..][0] = r(u0) cos 2 pi u1, [1] = r(u0) sin 2 pi u1, [2] = r(u2) cos 2 pi u3 (Box-Muller; the fourth
 * normal is dropped): every value finite, |z| <= 5.887.  Reads topo->num_nodes, num_graphs, graph_ptr only.  One launch for all
 * num_steps rows (the loop fills 128 steps at a time); the grid covers rows x atoms whatever the molecules' sizes. */
int agdiff_counter_noise(const agdiff_topo_t* topo, const int64_t* stream_id /* [G] */, uint64_t seed,
                         const int32_t* steps /* [S]: the counter word c1 of every row */, int32_t num_steps,
                         float* out /* [S][N][3] */, void* stream);

/* pos_perturbed = pos + pos_noise * sqrt(1 - a) / sqrt(a) with a = alpha_graph[graph of the atom]
 * (get_loss_diffusion, dualenc.py:306-312; alpha_graph[G] = alphas.index_select(0, time_step)). */
int agdiff_perturb_positions(const agdiff_topo_t* topo, const float* pos, const float* noise,
                             const float* alpha_graph, float* pos_out, void* stream);

/* Forward value of get_loss_diffusion (dualenc.py:329-395; evaluated under no_grad by scripts/train.py:160-170)
 * after agdiff_score_forward(pos_perturbed, AGDIFF_FWD_GLOBAL): d_gt / d_target per edge, global_mask, the four
 * eq_transforms and the per-atom squared errors.  loss: [3][N] = total, 2*global, 5*local. */
int agdiff_diffusion_loss(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                          const float* pos_gt, const float* pos_perturbed, const float* alpha_graph,
                          float* loss, void* stream);

/* One denoising step = agdiff_score_forward + agdiff_langevin_update (dualenc.py:478-545). */
int agdiff_langevin_step(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                         const agdiff_step_args_t* a, void* stream);

/* ---- evaluation (the step after the path) ------------------------------------------------------
 * get_rmsd_confusion_matrix (utils/evaluation/covmat.py:16-35): out[j][i] = GetBestRMS(gen_i, ref_j) over the atoms
 * listed in `atom_idx` (the reference removes hydrogens first, utils/chem.py:133-137) = the smallest, over the atom
 * mappings `perms`, of the RMSD after the optimal proper rotation + translation (rdkit rdMolAlign.GetBestRMS: every
 * substructure match of the molecule onto itself is aligned with AlignMol, no reflection, uniform weights).
 *   pos_ref [R][n][3], pos_gen [G][n][3]   conformers of ONE molecule with n atoms
 *   atom_idx [m]                            atoms that take part (m <= AGDIFF_RMSD_MAX_ATOMS), e.g. the heavy atoms
 *   perms [P][m] or null                    mapping p pairs generated atom atom_idx[k] with reference atom
 *                                           atom_idx[perms[p][k]]; null = the identity only (no symmetry: an upper bound
 *                                           of GetBestRMS)
 *   scratch [(R + G) * (3 m + 1)] floats    centred coordinates of the selected atoms (written by the call)
 *   out [R][G]
 * A conformer with a selected coordinate that is not finite (NaN, +inf or -inf) is +inf in its whole row (a reference)
 * or column (a generated one), in out and in out_mirror of agdiff_rmsd_matrix_hands, and every other entry keeps its
 * bits; the atoms that atom_idx does not list are never read. */
int agdiff_rmsd_matrix(const float* pos_ref, const float* pos_gen, const int32_t* atom_idx, const int32_t* perms,
                       int32_t R, int32_t G, int32_t n, int32_t m, int32_t P, float* scratch, float* out, void* stream);

/* Row and column minima of a confusion matrix [R][G] (covmat.py:135-136: rmsd_ref_min = min over generated,
 * rmsd_gen_min = min over references): row_min [R], col_min [G]. */
int agdiff_matrix_minima(const float* mat, int32_t R, int32_t G, float* row_min, float* col_min, void* stream);

/* ---- conformer ensembles (after the sampler): prune near-duplicates by symmetry-aware RMSD, superpose the rest ------
 * What rdkit's EmbedMultipleConfs(pruneRmsThresh=...) / AlignMolConformers do with a conformer set, for the 2 x num_refs
 * conformers per molecule that scripts/test.py:135-141 samples.  Three calls, no atomics, deterministic bit for bit.
 *
 * agdiff_rmsd_self: the G x G matrix of agdiff_rmsd_matrix(pos, pos) computed ONCE per pair.  For i < j the value is that
 * call's quantity with x = conformer i, y = conformer j (mapping p pairs atom atom_idx[k] of i with atom
 * atom_idx[perms[p][k]] of j), stored at [i][j] and mirrored to [j][i]; the diagonal is 0.  The mirror is the true
 * [j][i] value when `perms` is closed under inversion -- a group, as heavy_atom_automorphisms returns -- or null.
 * The launch covers the T (T + 1) / 2 upper-triangular 16 x 16 tiles only, T = ceil(G / 16).
 *   pos [G][n][3], atom_idx [m] (m <= AGDIFF_RMSD_MAX_ATOMS), perms [P][m] or null
 *   scratch [G * (3 m + 1)] floats     centred coordinates (written by the call)
 *   out [G][G] or null                 exactly symmetric
 *   bits or null                       the adjacency under `thresh` (>= 0): bit (i, j) = out[i][j] <= thresh, taken on the
 *                                      fp32 value as stored; diagonal set; bits of columns >= G zero.  Rows of 16-bit pieces,
 *                                      piece w of row i = columns 16 w .. 16 w + 15 (bit c = column 16 w + c), row pitch
 *                                      = 2 T bytes rounded up to 8; G rows; 8-byte aligned.  Read as little-endian 64-bit
 *                                      words, word l of a row holds columns 64 l .. 64 l + 63.
 * At least one of out / bits must be given.  A conformer with a selected coordinate that is not finite is +inf in its row and
 * its column, except on the diagonal, which stays 0; its bits follow out <= thresh like every other bit (clear for a finite
 * thresh, the diagonal set); every other entry and bit is unchanged. */
int agdiff_rmsd_self(const float* pos, const int32_t* atom_idx, const int32_t* perms, int32_t G, int32_t n, int32_t m,
                     int32_t P, float thresh, float* scratch, float* out, uint64_t* bits, void* stream);

/* The greedy leader algorithm in conformer order (pruneRmsThresh) over `bits` in the layout above: conformer i is kept iff
 * no KEPT j < i has bit (i, j); otherwise leader[i] is the smallest such j.  keep [G] (1 / 0), leader [G] (= i for a kept
 * conformer), count [G] (conformers led by i, itself included; 0 for a dropped one), n_kept [1].  One wave walks the rows in
 * order with the next rows already in flight.  G <= AGDIFF_PRUNE_MAX_CONFS, else AGDIFF_ERR_LIMIT. */
int agdiff_leader_prune(const uint64_t* bits, int32_t G, int32_t* keep, int32_t* leader, int32_t* count, int32_t* n_kept,
                        void* stream);

/* Taylor-Butina clustering (rdkit Butina.ClusterData) over `bits` in the layout above: which conformer families there are, how
 * populated each is, and which conformer sits in the middle of each.  The rule:
 *   - every conformer starts live; repeat until nobody is live:
 *       - among the live conformers take c with the largest neighbour count, ties to the LOWEST index;
 *       - the cluster of c is c itself plus every live j with bit (c, j);
 *       - the members of that cluster stop being live.
 *   - the neighbour count of i is the number of conformers j with bit (i, j) set,
 *       reorder = 1: over the conformers STILL LIVE when the choice is made -- the counts shrink as clusters are removed
 *                    (Butina's algorithm proper; ClusterData(reordering=True));
 *       reorder = 0: over ALL G conformers, counted once before the first choice (reordering=False): the leader walk of
 *                    agdiff_leader_prune run in the order (count descending, index ascending).
 * leader [G]: the centroid of each conformer's cluster (itself for a centroid); count [G]: the cluster size at a centroid, 0
 * elsewhere; rank [G]: the 0-based creation order of the conformer's cluster; n_clusters [1].  Every entry is written.
 * Bits in columns >= G are ignored (the last word is masked, the padding is not trusted) and the diagonal is taken as set, so
 * the centroid always leaves the live set: the outer loop is counted, at most G iterations.  `bits` is expected to be symmetric;
 * on an asymmetric matrix the partition is unspecified, and the call still ends within G iterations and writes only inside its
 * three arrays.  One workgroup, no global atomics, deterministic bit for bit.  A null pointer, `bits` not 8-byte aligned,
 * G < 0 or reorder outside {0, 1}: AGDIFF_ERR_ARG; G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT; G == 0: n_clusters = 0 and
 * no launch. */
int agdiff_butina_cluster(const uint64_t* bits, int32_t G, int32_t reorder, int32_t* leader, int32_t* count, int32_t* rank,
                          int32_t* n_clusters, void* stream);

/* MaxMin picking (farthest-point sampling; what rdkit's MaxMinPicker is used for) over the FLOAT matrix that agdiff_rmsd_self or
 * agdiff_tfd_matrix writes: a diverse subset of at most K conformers, the k-centre covering radius after every pick, and every
 * conformer's nearest pick.  dist is [G][G] fp32, contiguous.  Only the rows of picked conformers are ever read, so the rule is
 * defined by rows and symmetry is not required; the diagonal is never trusted (a picked column is not looked at).  The rule:
 *   - eligibility: every conformer starts eligible.  Whenever a pick p's row is read, every column j that is unpicked and still
 *     eligible is checked: if dist[p][j] is not a finite number >= 0 (NaN, +inf, -inf or negative), j becomes INELIGIBLE FOR GOOD.
 *     (That is what agdiff_rmsd_self stores for a conformer with a coordinate that is not finite: +inf across its row and column.)
 *     -0.0f counts as 0, and is taken as +0.0f.
 *   - pick 0 is `first`, as given; radius[0] = +inf.
 *   - after each pick p (its rank r), every eligible unpicked j is updated: if dist[p][j] < near[j] -- a strict < on the fp32
 *     values, near[j] = +inf before the first pick -- then near[j] = dist[p][j] and owner[j] = r.  On ties owner[j] stays with
 *     the EARLIER pick.
 *   - the candidate is the eligible unpicked j with the largest near[j], ties to the LOWEST index.
 *   - the candidate is picked iff fewer than K conformers are picked AND near[candidate] > stop (strict); then radius[r] =
 *     near[candidate] as it was when chosen.  A negative `stop` is no threshold.
 *   - the walk ends at the first candidate that is not picked, or when no candidate exists.
 * Outputs, every entry written:
 *   picks [K], radius [K]   in pick order; the entries from n_picked on are -1 and NaN
 *   owner [G]               the rank (index into picks) of each conformer's nearest pick, its own rank for a pick; -1 for an
 *                           ineligible conformer
 *   near [G]                the distance to that pick; 0 for a pick, NaN for an ineligible conformer
 *   n_picked [1]            the number of picks made (>= 1 for G > 0)
 *   cover [1]               the near of the last candidate, the one that was not picked; 0 when no candidate was left.  Every
 *                           eligible conformer is within `cover` of a pick.
 * Every float written is a copy of a matrix entry (or 0, +inf, NaN): nothing is computed, so everything is exact.  radius[1:] is
 * non-increasing and cover <= radius[n_picked - 1].  One workgroup, no global atomics, deterministic bit for bit; the outer loop
 * is counted, at most K iterations, one row read each.  `dist` needs 4-byte alignment only, and any G, odd ones included.
 * A null pointer or G < 0: AGDIFF_ERR_ARG; for G > 0, K outside [1, G], `first` outside [0, G) or a NaN `stop`: AGDIFF_ERR_ARG;
 * G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT (the argument errors come first); G == 0: n_picked = 0, cover = 0 and no launch.
 * Agreement with rdkit's MaxMinPicker is not claimed: that one draws its first pick at random, this one is deterministic. */
int agdiff_maxmin_pick(const float* dist, int32_t G, int32_t K, int32_t first, float stop, int32_t* picks, float* radius,
                       int32_t* owner, float* near, int32_t* n_picked, float* cover, void* stream);

/* K representative conformers with their populations: alternating k-medoids (Voronoi iteration) from K given seeds over the
 * same FLOAT matrix, dist [G][G] fp32, contiguous.  All sums and comparisons are made on a fixed-point image of the entries, so
 * no result depends on a summation order and everything below is exact.
 *   - validity: valid(x) = x >= 0.0f && x <= 4096.0f (AGDIFF_KMEDOIDS_MAX_DIST).  NaN, negative values, +-inf and anything above
 *     the cap are not valid; -0.0f is valid and counts as 0.
 *   - the quantiser: Q(x) = uint64(rint((double)x * 2^28)), rounding half to even, for a valid x (the product is exact in fp64);
 *     Q(x) = 2^40 for an entry that is not valid: "as far as the cap".  A sum of at most 4096 such terms is <= 2^52, so
 *     sum << 12 | index fits 64 bits and a total divided by 2^28 is exact in fp64.
 *   - eligibility: conformer j is eligible iff j == init[0] or valid(dist[init[0]][j]): one row decides (agdiff_rmsd_self writes
 *     +inf across the row and column of a conformer with a coordinate that is not finite).  An ineligible conformer takes no
 *     further part.  Among eligible conformers an entry that is not valid counts as 2^40.
 *   - seeds: init [K] holds the medoids of rank 0 .. K - 1.  The kernel checks them: a seed outside [0, G), a duplicate seed or an
 *     ineligible seed gives status = 2 and nothing else is computed.
 *   - assign: a medoid belongs to its own rank, with near 0.  Every other eligible j goes to the rank r with the smallest
 *     Q(dist[medoid_r][j]), ties to the LOWEST rank.  The rows read are the medoids' rows: symmetry is not required and the
 *     diagonal is never read.
 *   - update: for every cluster r and every member i, cost_i = the sum of Q(dist[i][j]) over the members j != i, taken along
 *     row i.  The new medoid is the member with the smallest cost, ties to the LOWEST index -- but if the incumbent medoid's
 *     cost equals that minimum, THE INCUMBENT STAYS.  With this the total cost falls strictly at every update that changes
 *     anything, and the walk cannot cycle.
 *   - the loop: assign and update repeat until an update changes no medoid (status = 0) or max_iter updates have been made
 *     (status = 1).  n_iter is the number of updates made, counting the one that changed nothing.  The returned labels are
 *     always the assignment to the returned medoids: after a status = 1 stop one more assign runs.  Ranks never change:
 *     medoids[r] descends from init[r].
 * Outputs, every entry written:
 *   medoids [K]   the medoid of each rank
 *   labels [G]    the rank of each conformer's cluster; -1 for an ineligible conformer
 *   near [G]      a copy of dist[medoid][j] as stored, -0.0f written as +0.0f; 0 for a medoid, NaN for an ineligible conformer
 *   size [K]      the number of members of each cluster
 *   within [K]    each cluster's sum of Q(near) / 2^28
 *   cost [1]      the total over all clusters
 *   n_iter [1]    the number of updates made
 *   status [1]    0 converged, 1 stopped at max_iter, 2 a bad seed
 * On status = 2: medoids all -1, labels all -1, near all NaN, size 0, within 0, cost 0 and n_iter 0.
 * work: caller-provided scratch of AGDIFF_KMEDOIDS_WORK_BYTES, 8-byte aligned; its contents are ignored on entry and unspecified
 * on return.  `dist` needs 4-byte alignment only, and any G, odd ones included.
 * An iteration is three launches -- assign (columns across threads, a loop over the K medoid rows), member costs (one wave per
 * candidate row), choose (per-cluster arg-min over the keys cost << 12 | index, the incumbent rule, the done flag) -- and the
 * call enqueues them for max_iter iterations, plus the seed check, the final assign and the sums.  Every launch reads a
 * device-side `done` flag first and returns at once when it is set.  No cooperative launch, no workgroup waits on another, no
 * atomics on global memory; every loop is counted; deterministic bit for bit.
 * A null pointer or G < 0: AGDIFF_ERR_ARG; for G > 0, K outside [1, G] or max_iter outside [1, AGDIFF_KMEDOIDS_MAX_ITER]:
 * AGDIFF_ERR_ARG; `work` not 8-byte aligned: AGDIFF_ERR_ARG; G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT (the argument errors
 * come first); G == 0: n_iter = 0, status = 0, cost = 0 and no launch.
 * This is not PAM's swap phase: a local optimum that depends on the seeds (PAM is agdiff_pam_build + agdiff_pam_swap, below).
 * Agreement with any other package's k-medoids is not claimed. */
int agdiff_kmedoids(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t max_iter,
                    int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,
                    double* cost, int32_t* n_iter, int32_t* status, uint64_t* work, void* stream);

/* Seed-independent representatives: PAM (Kaufman & Rousseeuw), a greedy BUILD that needs no seeds and a steepest-descent SWAP
 * that tries every (medoid, non-medoid) exchange, so that a medoid can leave its cluster altogether.  Same FLOAT matrix, dist
 * [G][G] fp32, contiguous; valid(x), Q(x) and the cap are agdiff_kmedoids'.  All arithmetic is on integers: Q values, sums <= 2^52,
 * signed differences in int64.  The diagonal is never read and counts as 0.  Symmetry is not required: "the distance from medoid
 * or candidate c to o" is always dist[c][o], along row c.
 *   - eligibility: both calls take an explicit `anchor`.  Conformer j is eligible iff j == anchor or valid(dist[anchor][j]).  An
 *     ineligible conformer takes no part and is never a candidate.  Among eligible conformers an entry that is not valid counts
 *     as 2^40.
 *   - the state of a medoid set, for each eligible o: n(o) is the nearest medoid's rank, ties to the LOWEST rank, and a medoid
 *     belongs to its own rank with distance 0 even if a lower-rank medoid is at Q = 0 (agdiff_kmedoids' assign); dn(o) is that Q;
 *     ds(o) is the smallest Q over the ranks other than n(o), infinite for K = 1: min(ds, x) = x.
 * agdiff_pam_build makes K medoids in rank order from nothing:
 *   - rank 0 is the eligible c with the smallest sum over the eligible o != c of Q(dist[c][o]), ties to the lowest index;
 *   - each further rank is the eligible non-medoid c with the largest gain(c) = dn(c) + the sum over the eligible non-medoids
 *     o != c of max(dn(o) - Q(dist[c][o]), 0), ties to the lowest index; a gain of 0 still picks;
 *   - after each pick dn(o) = min(dn(o), Q(dist[c][o])).  (With dn = 2^40 before the first pick, rank 0 is the same rule.)
 *   - K above the number of eligible conformers or `anchor` outside [0, G): status = 2.  Otherwise status = 0 and n_swaps = 0.
 * agdiff_pam_swap is steepest descent from the K seeds init [K] (checked as agdiff_kmedoids checks them, eligibility under
 * `anchor`: a seed or an anchor outside [0, G), a duplicate or an ineligible seed gives status = 2).  One iteration computes for
 * every candidate c (eligible, not a medoid), with x(o) = Q(dist[c][o]) and x(c) = 0:
 *     gain(c)     = the sum over all eligible o of dn(o) - min(dn(o), x(o))
 *     corr(c, r)  = the sum over the o with n(o) == r of min(ds(o), x(o)) - min(dn(o), x(o))
 *     delta(c, r) = corr(c, r) - gain(c)
 *   delta(c, r) is exactly the change of the total cost when c replaces the medoid of rank r and everyone is reassigned.  The
 *   iteration takes the smallest delta, ties to the lowest candidate index, then to the lowest rank.  If it is < 0 (strictly),
 *   medoids[r] = c -- the rank is kept, so medoids[r] descends from init[r] by exchanges --, n_swaps is incremented and the state
 *   is recomputed; otherwise the walk stops with status = 0.  With no candidate (K == the number of eligible conformers): status
 *   0 with 0 swaps.  After max_swaps swaps, with a negative delta possibly left and not looked for: status = 1 (so max_swaps = 0
 *   returns the seeds' assignment with status 1).  The cost falls strictly with every swap, so the walk cannot cycle.  The rule
 *   is memoryless: calling again with the returned medoids as init and the same anchor continues the same walk bit for bit.
 * Outputs of both, agdiff_kmedoids', every entry written in every case: medoids [K], labels [G], near [G], size [K], within
 * [K], cost [1]; n_swaps [1] in n_iter's place; status [1].  labels and near are always the assignment to the returned medoids.
 * On status = 2 the fill is agdiff_kmedoids'.
 * work: caller-provided scratch of AGDIFF_PAM_WORK_BYTES, 8-byte aligned; its contents are ignored on entry and unspecified on
 * return.  `dist` needs 4-byte alignment only, and any G, odd ones included.
 * A swap iteration is three launches -- the state (agdiff_kmedoids' assign keeping the second-best too), the candidates (row c
 * is streamed once: the gain in registers, corr in K uint64 bins in LDS, one row per wave for K <= 1024 and one per workgroup
 * above, as agdiff_silhouette; then the arg-min over the bins, one record per candidate), the choose (one workgroup: the arg-min
 * of the records, applied or not) -- and the call enqueues them for max_swaps iterations, plus the seed check, the final state
 * and the sums.  BUILD is the candidates' launch without bins and a pick per rank: 2 K + 3 launches.  Every launch of a loop reads
 * a device-side `done` flag first and returns at once when it is set.  No cooperative launch, no workgroup waits on another, no
 * atomics on global memory; every loop is counted; deterministic bit for bit.
 * A null pointer or G < 0: AGDIFF_ERR_ARG; for G > 0, K outside [1, G] or max_swaps outside [0, AGDIFF_PAM_MAX_SWAPS]:
 * AGDIFF_ERR_ARG; `work` not 8-byte aligned: AGDIFF_ERR_ARG; G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT (the argument errors
 * come first); G == 0: n_swaps = 0, status = 0, cost = 0 and no launch.
 * Not built: FasterPAM's eager variant (several swaps per pass), CLARA / CLARANS sampling, k-means++ / LAB seeding.  Agreement
 * with any other package's PAM is by the definition only. */
int agdiff_pam_build(const float* dist, int32_t G, int32_t K, int32_t anchor,
                     int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,
                     double* cost, int32_t* n_swaps, int32_t* status, uint64_t* work, void* stream);
int agdiff_pam_swap(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t anchor, int32_t max_swaps,
                    int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,
                    double* cost, int32_t* n_swaps, int32_t* status, uint64_t* work, void* stream);

/* How good is a clustering, and how many families are there: the silhouette coefficient (Rousseeuw 1987) of every conformer of
 * a GIVEN clustering over the same FLOAT matrix, dist [G][G] fp32, contiguous, made exact the way agdiff_kmedoids is: all sums
 * are made on the fixed-point image of the entries, so no result depends on a summation order and everything below is exact.
 *   - validity and the quantiser are agdiff_kmedoids': valid(x) = x >= 0.0f && x <= 4096.0f; Q(x) = uint64(rint((double)x * 2^28)),
 *     rounding half to even, for a valid x and Q(x) = 2^40 for an entry that is not valid; -0.0f counts as 0.
 *   - labels [G]: labels[j] == -1 means conformer j is LEFT OUT: it takes no part and is never read as a column.
 *     0 <= labels[j] < K means j is a member of rank labels[j].  Any other value gives status = 2 and nothing else is computed.
 *     The check is made on the device: the host never reads `labels`.
 *   - sizes: size[c] is the number of members of rank c.  A rank with no member is allowed (K may exceed the ranks used, and K
 *     may exceed G); an EMPTY RANK IS NEVER anybody's other cluster.
 *   - sums: for a member i and a rank c, S_c(i) = the sum of Q(dist[i][j]) over the members j != i of rank c, taken along ROW i.
 *     Symmetry is not required and the diagonal is never read.  The sums are uint64 sums of integers, <= 4096 * 2^40 = 2^52.
 *   - means, in fp64 and in units of 2^-28, each ONE correctly rounded division of two exactly converted integers:
 *       ma  = (double)S_own / (double)(size_own - 1), and 0 when size_own == 1
 *       m_c = (double)S_c / (double)size[c]
 *   - mb is the smallest m_c over the non-empty ranks c != own and other[i] is that rank, ties to the LOWEST rank.  With no
 *     such rank other[i] = -1 and b[i] = NaN.
 *   - the coefficient: s(i) = 0 when size_own == 1, when there is no other non-empty rank, or when max(ma, mb) == 0; otherwise
 *     s(i) = (mb - ma) / max(ma, mb): one fp64 subtraction and one fp64 division.
 *   - a[i] = ma * 2^-28 and b[i] = mb * 2^-28, exact scalings.  A left-out conformer gets a, b and s NaN and other -1.
 *   - aggregates: T(i) = (int64)rint(s(i) * 2^40) (the product is exact); cluster_mean[c] = ((double)(the sum of T(i) over the
 *     members of c) / (double)size[c]) * 2^-40, NaN for an empty rank; mean[0] is the same quantity over all members, NaN when
 *     there are none.  The sums of T are integer sums, <= 2^52 in magnitude.
 * Outputs, every entry written in every case:
 *   a [G], b [G], s [G]   fp64: the mean distance to the own cluster's other members, to the nearest other cluster, the coefficient
 *   other [G]             the rank of that nearest other cluster, -1 for none
 *   size [K]              the members of each rank
 *   cluster_mean [K]      the mean coefficient of each rank's members
 *   mean [1]              the mean coefficient of all members
 *   status [1]            0, or 2 for a bad label
 * On status = 2: a, b, s, cluster_mean and mean NaN, other all -1 and size 0.
 * work: caller-provided scratch of AGDIFF_SILHOUETTE_WORK_BYTES, 8-byte aligned; its contents are ignored on entry and unspecified
 * on return.  `dist` needs 4-byte alignment only, and any G, odd ones included.
 * Three launches: the label check and the sizes (one workgroup), the rows (row i is streamed once into K uint64 bins in LDS; one
 * row per wave for K <= 1024, one row per workgroup above, so that a workgroup's bins take at most 32 KB), the aggregates (one
 * workgroup).  What crosses lanes is an integer or a (mean, rank) pair compared under a total order.  No cooperative launch, no
 * workgroup waits on another, no atomics on global memory; every loop is counted; deterministic bit for bit.
 * A null pointer or G < 0: AGDIFF_ERR_ARG; K outside [1, AGDIFF_PRUNE_MAX_CONFS]: AGDIFF_ERR_ARG; `work` not 8-byte aligned:
 * AGDIFF_ERR_ARG; G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT (the argument errors come first); G == 0: status = 0, size 0,
 * cluster_mean and mean NaN, and no launch.
 * This is the full silhouette, O(G^2): not the simplified (medoid-based) one, and neither a gap statistic nor Davies-Bouldin.
 * Agreement with scikit-learn's silhouette_samples is by definition only, not bit for bit. */
int agdiff_silhouette(const float* dist, int32_t G, int32_t K, const int32_t* labels,
                      double* a, double* b, double* s, int32_t* other,
                      int32_t* size, double* cluster_mean, double* mean, int32_t* status,
                      uint64_t* work, void* stream);

/* The conformer family tree: agglomerative (hierarchical) linkage clustering over the same FLOAT matrix, dist [G][G] fp32,
 * contiguous -- one tree per molecule, and any cut of it is a clustering, so no threshold and no count is needed before it runs.
 * valid(x), Q(x) and the cap are agdiff_kmedoids'.  ONLY THE STRICT UPPER TRIANGLE IS READ: the pair {i, j} with i < j takes
 * Q(dist[i][j]); the diagonal and the lower triangle are never read.
 *   - eligibility is agdiff_pam_build's, with an explicit `anchor`: conformer j is eligible iff j == anchor or
 *     valid(dist[anchor][j]), read along row `anchor` (the one place where an entry at or below the diagonal is read).  M is the
 *     number of eligible conformers.  Among eligible conformers an entry that is not valid counts as 2^40.  An ineligible
 *     conformer takes no part.
 *   - clusters: every eligible conformer starts as a cluster.  A cluster is named by its lowest member index, its SLOT.
 *   - the pair weight W(A, B), a uint64: method AGDIFF_LINKAGE_SINGLE the minimum of Q over the pairs between A and B,
 *     AGDIFF_LINKAGE_COMPLETE the maximum, AGDIFF_LINKAGE_AVERAGE (UPGMA) the SUM, at most 2^22 pairs x 2^40 = 2^62.
 *   - the key of a pair of clusters, an fp64 in units of 2^-28: (double)W for single and complete, which is exact; for average
 *     (double)W / (double)(|A| |B|): W converted round-to-nearest-even (exact below 2^53), the count converted exactly, then ONE
 *     correctly rounded division, as agdiff_silhouette makes its means.
 *   - a merge: among all pairs of live clusters with slots a < b the smallest key is taken, TIES TO THE LOWEST a, THEN TO THE
 *     LOWEST b.  The union takes slot a and b dies.  For every other live cluster c, W(a, c) becomes the min, the max or the sum
 *     of W(a, c) and W(b, c): integer arithmetic only.  Merge t records left[t] = a, right[t] = b, height[t] = key * 2^-28 (an
 *     exact scaling) and size[t] = |A| + |B|.  There are M - 1 merges; the entries t >= M - 1 are -1, -1, NaN and 0.
 *   - the leaf order: a merge puts b's leaves after a's.  order[j] is conformer j's position, 0 .. M - 1, in the resulting
 *     left-to-right order; -1 for an ineligible conformer.  (A cluster's list always starts at its slot, so a merge is
 *     next[tail[a]] = b; tail[a] = tail[b].)
 *   - HEIGHTS ARE NOT PROMISED MONOTONE.  In exact arithmetic all three linkages are monotone; with the one rounding of `average`
 *     above 2^53 an inversion of one ulp cannot be excluded, so nothing here is defined through monotonicity.  It is guaranteed
 *     whenever every sum stays below 2^53: always for single and complete, and for average e.g. when every entry is <= 1 (2^28)
 *     or the largest product |A| |B| times the largest entry stays below 2^25.
 * agdiff_linkage outputs, every entry written in every case: left [G], right [G], height [G] (fp64), size [G], order [G],
 * status [1]: 0, or 2 for an `anchor` outside [0, G), judged on the device: everything is then filled as on an empty tree (-1,
 * -1, NaN, 0; order all -1).
 * work: caller-provided scratch of 8 G G + AGDIFF_LINKAGE_WORK_FIXED_BYTES bytes, 8-byte aligned; its contents are ignored on
 * entry and unspecified on return.  `dist` needs 4-byte alignment only, and any G, odd ones included.
 * The working state is a uint64 square of which the upper triangle is used and, per slot, the size, a live flag and (nn_key,
 * nn_idx): the smallest key of row k over the live j > k, ties to the lowest j.  Launches: the head (one workgroup: the anchor,
 * eligibility, the fills), the rows (one wave per row: W from Q and every row's nearest neighbour), then G - 1 times two
 * launches -- choose (one workgroup: the arg-min of (nn_key, k) over the live rows, the merge record, the list splice) and
 * update (one wave per slot: wave a rewrites and rescans row a, a wave c < a rewrites (c, a) and rescans only when its nearest
 * neighbour was a or b, a wave c > a rescans only when it was b; no wave reads what another writes in the same launch) -- and
 * one that ranks the list into `order`.  Every launch of the loop reads a device-side merge counter first and returns at once
 * past M - 1.  No cooperative launch, no workgroup waits on another, no atomics on global memory; every loop is counted;
 * deterministic bit for bit.
 *
 * agdiff_linkage_cut turns the tree into a clustering.  It reads the tree (left, right, height, order as agdiff_linkage wrote
 * them; order[j] >= 0 says who is eligible), not the working matrix, and takes `count` K >= 1 and `stop_height` T, +inf or
 * valid(T).  The merges are applied in order, t = 0, 1, ..., while more than K clusters remain AND height[t] <=
 * Q(T) * 2^-28 (no bound for +inf); the first merge that fails either test ends it, whatever comes later.  count = 1 with
 * T = +inf is the whole tree; count >= M applies nothing.
 *   - the clusters are ranked by ascending slot; labels [G] is the rank, -1 for an ineligible conformer: agdiff_silhouette's
 *     input as it stands; n_clusters [1];
 *   - medoids [G]: medoids[c] is the member with the smallest sum of Q(dist[i][j]) over the members j != i along row i, ties to
 *     the lowest index: agdiff_kmedoids' update without an incumbent (its member-cost pass and per-cluster arg-min);
 *   - near [G], size [G], within [G], cost [1] as agdiff_kmedoids defines them, relative to `medoids`;
 *   - the arrays indexed by rank are [G] long and filled up to n_clusters; the rest is -1 (medoids), 0 (size) or 0.0 (within);
 *   - status [1]: 0, or 2 for an applied merge that is not one (not 0 <= left < right < G between eligible conformers): the
 *     fill is then agdiff_kmedoids' and n_clusters = 0.
 * work: caller-provided scratch of AGDIFF_LINKAGE_CUT_WORK_BYTES, 8-byte aligned.  Four launches: the cut (one workgroup:
 * parent[b] = a of the applied merges in LDS, one thread per conformer chasing parents to the root -- a parent has a lower index,
 * so the loop is counted by G --, a prefix sum over the root flags for the ranks), the member costs, the per-cluster arg-min
 * with near, and agdiff_kmedoids' sums.
 * Both: a null pointer, G < 0, a method outside 0 .. 2, count < 1, a T that is NaN, negative or finite above the cap, or a
 * `work` that is not 8-byte aligned: AGDIFF_ERR_ARG; G > AGDIFF_PRUNE_MAX_CONFS: AGDIFF_ERR_LIMIT (the argument errors come
 * first); G == 0: no launch, status = 0 (and n_clusters = 0, cost = 0).
 * Not built: Ward, centroid and median linkage (the matrix is not Euclidean), optimal leaf ordering.  Agreement with
 * scipy.cluster.hierarchy.linkage is by the definition and on tie-free input only: its tie order is its own. */
int agdiff_linkage(const float* dist, int32_t G, int32_t method, int32_t anchor,
                   int32_t* left, int32_t* right, double* height, int32_t* size, int32_t* order, int32_t* status,
                   uint64_t* work, void* stream);
int agdiff_linkage_cut(const float* dist, int32_t G, const int32_t* left, const int32_t* right, const double* height,
                       const int32_t* order, int32_t count, float stop_height,
                       int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within,
                       double* cost, int32_t* n_clusters, int32_t* status, uint64_t* work, void* stream);

/* Rigid superposition (rdkit AlignMolConformers: atoms keep their labels, identity mapping): for each conformer the proper
 * rotation R and translation that minimise the RMSD to `target` over the atoms `atom_idx` (Horn's quaternion, fp64), applied
 * to ALL n atoms: out = R (x - c_x) + c_target, so hydrogens ride along.  No reflection: a mirror image stays apart.  When
 * the best rotation is not unique (collinear atoms) one of the maximisers is taken.
 *   pos [G][n][3], atom_idx [m], target [n][3], out [G][n][3] (not overlapping pos),
 *   rmsd [G] or null: the RMSD over atom_idx between out, as stored, and target */
int agdiff_align_conformers(const float* pos, const int32_t* atom_idx, const float* target, int32_t G, int32_t n, int32_t m,
                            float* out, float* rmsd, void* stream);

/* ---- handedness ------------------------------------------------------------------------------------------------------
 * The score network sees atom types, bonds and distances only, so the sampler draws a molecule and its mirror image with
 * equal probability.  Three calls, no atomics, deterministic bit for bit.
 *
 * agdiff_rmsd_matrix_hands: agdiff_rmsd_matrix with a second matrix.  out_proper [R][G] is bit for bit what agdiff_rmsd_matrix
 * writes; out_mirror [R][G] is the same quantity for the generated conformer inverted through its centroid (its mirror
 * image), minimised over the same mappings: sqrt(max(0, min_p (|X|^2 + |Y|^2 + 2 lambda_min(K_p)) / m)).  K is linear in the
 * cross-covariance S and the inversion turns S into -S, so both values come from one diagonalisation per (pair, mapping).
 * Arguments as for agdiff_rmsd_matrix; out_proper and out_mirror must not overlap. */
int agdiff_rmsd_matrix_hands(const float* pos_ref, const float* pos_gen, const int32_t* atom_idx, const int32_t* perms,
                             int32_t R, int32_t G, int32_t n, int32_t m, int32_t P, float* scratch, float* out_proper,
                             float* out_mirror, void* stream);

/* Parity of tetrahedral stereocentres, per conformer.
 *   pos [G][n][3]
 *   quads [C][4] int32     the four bonded neighbours (a, b, c, d) of each centre, in ascending atom index
 *   target [C] int8        +1 / -1: the parity the centre should have; 0: do not check   (quads / target may be null when C = 0)
 *   vol [G][C] or null     (p_b - p_a) . ((p_c - p_a) x (p_d - p_a)) in fp64 from the fp32 positions, stored as fp32
 *   verdict [G] int32      +1: every checked centre has its target parity (also: C = 0, nothing checked)
 *                          -1: every checked centre is inverted -- the conformer is the mirror image
 *                           0: the checked centres disagree, or one of them has parity 0: reflection cannot fix it
 * The parity of a centre is the sign of the fp64 volume, 0 when that is zero or not finite.  A quad naming an atom outside
 * [0, n) counts as volume 0 and reads nothing. */
int agdiff_chiral_verdict(const float* pos, const int32_t* quads, const int8_t* target, int32_t G, int32_t n, int32_t C,
                          float* vol, int32_t* verdict, void* stream);

/* Mirror images in place: for every conformer g with flags[g] != 0 (int32 [G]), p <- (float)(2 c - (double)p) with c the fp64
 * centroid of ALL n atoms.  Inversion through the centroid keeps every distance and the centroid.  Conformers with
 * flags[g] == 0 are neither read nor written.  pos [G][n][3]. */
int agdiff_mirror_conformers(float* pos, const int32_t* flags, int32_t G, int32_t n, void* stream);

/* E/Z of double bonds, judged and repaired in place: the bond types the score network sees do not say which isomer a C=C, C=N or
 * N=N is, and the sampler draws either.  The host finds the stereogenic double bonds and the atoms on one side of each
 * (agdiff_amd/ezbonds.py).
 *   pos [G][n][3]             read and written
 *   quads [D][4] int32        (a, i, j, d): the double bond i - j, a neighbour a of i and a neighbour d of j
 *   target [D] int8           +1: a and d on opposite sides (trans); -1: on the same side (cis); 0: do not judge
 *   side_ptr [D + 1], side_idx   CSR: the atoms that turn with one end of bond c, entries in [0, n) (NOT checked against the graph
 *                             here: the caller does); an empty row: judge, do not flip.  side_idx may be null when every row is empty
 *   state [G][D] int8         +1 right, -1 wrong, 0 undecided or target 0 -- from the positions as they are when the bond's turn
 *                             comes (the bonds are walked in row order), that is BEFORE this bond's own flip
 *   flipped [G] int32 or null the number of flips applied to the conformer (not written when G = 0 or D = 0)
 * The parity of a bond is read from n1 . n2 = |n1| |n2| cos(phi) of agdiff_torsion_angles' formula (fp64 from the fp32 positions):
 * +1 when it is negative (|phi| > 90 degrees), -1 when positive, 0 when it or a normal is zero or a coordinate is not finite.  A
 * quad naming an atom outside [0, n) reads nothing and gives state 0.
 * A bond with state -1 and a side row is flipped: every listed atom p is turned by 180 degrees about the axis through p_i along
 * u = (p_j - p_i) / |p_j - p_i|, p' = 2 (p_i + u (u . (p - p_i))) - p in fp64, stored as fp32.  Atoms i and j are skipped when
 * listed and stay bit for bit, as does a listed atom with a coordinate that is not finite.  A 180 degree rotation of a rigid side
 * keeps every bond length, every distance within each side and every tetrahedral parity (it is a proper rotation, not a
 * reflection); it negates cos(phi) of that one bond and leaves the other tagged bonds' dihedrals alone when the bonds are
 * bridges (the four atoms of any other quad lie on one side of the cut).  It CAN create contacts between the two sides: that is
 * why the driver runs the flip before the repairs and the checks.  A conformer without a wrong bond that has a side row is not
 * written at all.  No limit on n or D.  One wave per conformer, a workgroup barrier after each flip; deterministic. */
int agdiff_flip_double_bonds(float* pos /* [G][n][3], in place */, const int32_t* quads /* [D][4] */, const int8_t* target /* [D] */,
                             const int32_t* side_ptr /* [D + 1] */, const int32_t* side_idx, int32_t G, int32_t n, int32_t D,
                             int8_t* state /* [G][D] */, int32_t* flipped /* [G] or NULL: flips applied */, void* stream);

/* ---- torsion fingerprint deviation -----------------------------------------------------------------------------------
 * The second standard metric between conformers next to the RMSD: the mean circular difference of the rotatable bonds'
 * dihedrals, in [0, 1] and independent of the molecule's size (rdkit Chem.TorsionFingerprints.GetTFDBetweenConformers /
 * GetTFDMatrix, which the reference never calls; rdkit's distance-from-centre weights are not built, a caller passes weights; the
 * ring terms are opt-in, further down: agdiff_ring_coords, agdiff_tfd_matrix_terms).  The host finds the torsions
 * (agdiff_amd/torsions.py).  Two calls, no atomics, deterministic bit for bit.
 *
 * agdiff_torsion_angles: what rdkit's rdMolTransforms.GetDihedralRad gives for every quad of every conformer.
 *   pos [G][n][3]
 *   quads [Q][4] int32     atoms (a, u, v, b) of each column: the bond u - v, a neighbour a of u and a neighbour b of v (may be
 *                          null when Q = 0)
 *   out [G][Q]             theta = atan2(|b2| (b1 . n2), n1 . n2) in radians in [-pi, pi], with b1 = p_u - p_a, b2 = p_v - p_u,
 *                          b3 = p_b - p_v, n1 = b1 x b2, n2 = b2 x b3; fp64 from the fp32 positions, stored as fp32.  The
 *                          mirror image has -theta; theta(a, u, v, b) = theta(b, v, u, a).  NaN when |n1|^2 or |n2|^2 is zero
 *                          or a coordinate is not finite.  A quad naming an atom outside [0, n) gives NaN and reads nothing.
 * One wave per conformer, lanes over the columns. */
int agdiff_torsion_angles(const float* pos, const int32_t* quads, int32_t G, int32_t n, int32_t Q, float* out, void* stream);

/* agdiff_tfd_matrix: what GetTFDMatrix (self) and GetTFDBetweenConformers (cross) give, over angle tables of the call above.
 *   ang_x [R][Q], ang_y [G][Q]   angle tables of the same molecule (the same table for a self matrix); Q <= AGDIFF_TFD_MAX_COLUMNS
 *   tmap [P][T] int32            P >= 1 mappings of the T <= Q torsions onto columns, entries in [0, Q) (NOT checked here: the
 *                                caller does).  Row 0: each torsion's own column; row p: the column that holds the image of
 *                                torsion t under the molecule's p-th symmetry.
 *   w [T] or null                weights > 0; null = uniform
 *   delta(a, b) = min(|a - b|, 2 pi - |a - b|) in fp64 from the stored fp32 angles, pi when either is NaN
 *   S_p(x -> y) = sum_t w[t] delta(x[tmap[0][t]], y[tmap[p][t]]) / (pi sum_t w[t]),  t ascending, fp64
 *   out [R][G] or null           min_p min(S_p(x -> y), S_p(y -> x)) as fp32 -- both directions, because row 0's choice of
 *                                neighbours is not carried along by the symmetries and one direction alone is not symmetric
 *                                in (x, y).  T = 0 (a rigid molecule): 0.
 *   out_mirror [R][G] or null    the same with every angle of y negated: the TFD to y's mirror image.  Not overlapping out.
 *   bits or null                 the adjacency out <= thresh (>= 0) on the fp32 value as stored (computed whether or not out is
 *                                given), in exactly the layout of agdiff_rmsd_self: R rows of 16-bit pieces, row pitch
 *                                2 ceil(G / 16) bytes rounded up to 8, bits of columns >= G zero; 8-byte aligned.
 * With ang_x == ang_y the matrices are exactly symmetric and the diagonal of out is 0 where a conformer's angles are not NaN.
 * At least one of the three outputs must be given.  One workgroup per 16 x 16 tile of pairs, the 32 angle rows in LDS. */
int agdiff_tfd_matrix(const float* ang_x, const float* ang_y, const int32_t* tmap, const float* w, int32_t R, int32_t G,
                      int32_t Q, int32_t T, int32_t P, float thresh, float* out, float* out_mirror, uint64_t* bits,
                      void* stream);

/* ---- ring conformations ----------------------------------------------------------------------------------------------
 * The rotatable bonds above are bridges, so the TFD does not see a ring: chair and twist-boat cyclohexane are "the same
 * conformer".  Two opt-in calls: the shape of every ring of every conformer (the ring torsion value of Schulz-Gasch et al. 2012
 * and the Cremer-Pople puckering coordinates), and the TFD over a term list that holds rings next to bonds.  The host finds the
 * rings (agdiff_amd/rings.py: the chordless cycles of 4 .. 12 heavy atoms; a caller may name others).  rdkit is not a
 * dependency and agreement with its TFD is NOT claimed (it is believed not to cap a term at 1).  No atomics, deterministic bit
 * for bit.
 *
 * agdiff_ring_coords:
 *   pos [G][n][3]
 *   ring_ptr [Rg + 1] int32   ring r holds the atoms ring_idx[ring_ptr[r] .. ring_ptr[r + 1]) in walking order, N_r of them,
 *                             4 <= N_r <= AGDIFF_RING_MAX_ATOMS; ring_ptr[0] = 0.  DEVICE memory, like every table here; the
 *                             launcher reads the Rg + 1 words back to check the sizes (one stream synchronisation: the call
 *                             cannot be captured into a graph) and returns AGDIFF_ERR_LIMIT for a ring of fewer than 4 or more
 *                             than AGDIFF_RING_MAX_ATOMS atoms, AGDIFF_ERR_ARG when ring_ptr[0] != 0.
 *   ring_idx [ring_ptr[Rg]]   atom indices.  A ring that names an atom outside [0, n) reads nothing and has NaN in all its numbers.
 *   tau [G][Rg] or null       (1 / N) sum_j |theta(r_j, r_j+1, r_j+2, r_j+3)|, indices mod N, j ascending, theta exactly the
 *                             dihedral of agdiff_torsion_angles (fp64 from the fp32 positions); in [0, pi], stored as fp32; NaN
 *                             when one of the N dihedrals is NaN.  Invariant under the start atom, the walking direction, rigid
 *                             motion AND reflection.  It cannot tell a chair from its ring-flipped chair: only the sign of q_3 can.
 *   Cremer-Pople (J. Am. Chem. Soc. 97, 1354 (1975)), all in fp64, every sum j ascending, stored as fp32:
 *     c = mean r_j, d_j = r_j - c, R' = sum d_j sin(2 pi j / N), R'' = sum d_j cos(2 pi j / N), n = R' x R'' / |R' x R''|,
 *     z_j = d_j . n;  for m = 2 .. floor((N - 1) / 2):  q_m cos(phi_m) =  sqrt(2 / N) sum z_j cos(2 pi m j / N),
 *                                                       q_m sin(phi_m) = -sqrt(2 / N) sum z_j sin(2 pi m j / N),
 *     q_m >= 0, phi_m in [0, 2 pi) (a phase that the fp32 store would round up to 2 pi is stored as 0); for even N the signed
 *     q_(N/2) = sqrt(1 / N) sum (-1)^j z_j.  Every trig argument is sincospi(((2 m j) mod 2N) / N): exact at the symmetric points.
 *     sum_m q_m^2 (+ q_(N/2)^2) = Q^2.  Amplitudes do not depend on where and which way the ring is walked; phases do.
 *   amp [G][Rg] or null       the total amplitude Q = sqrt(sum z_j^2)
 *   pucker [G][K] or null     K = ring_ptr[Rg] - 3 Rg: ring r's N_r - 3 numbers start at ring_ptr[r] - 3 r, in the order
 *                             q_2, phi_2, ..., q_M, phi_M[, q_(N/2)]
 *   amp and pucker of a ring are NaN when |R' x R''|^2 is zero or one of its coordinates is not finite.
 * At least one output must be given; G = 0 or Rg = 0 launches nothing.  One wave per conformer, the lanes over the (ring,
 * position) slots: a slot's dihedral, then one lane per ring for the sums that need the whole ring, then a slot per mode. */
int agdiff_ring_coords(const float* pos, const int32_t* ring_ptr, const int32_t* ring_idx, int32_t G, int32_t n, int32_t Rg,
                       float* tau, float* amp, float* pucker, void* stream);

/* agdiff_tfd_matrix_terms: agdiff_tfd_matrix over value tables whose terms have a scale and a parity of their own -- the table of a
 * conformer is its Q dihedral columns followed by its ring columns tau_r, the term list the T rotatable bonds followed by the
 * rings.  Arguments, tiling, bit layout and output rules are agdiff_tfd_matrix's (Q and T count the ring columns and terms), plus
 *   scale [T] float > 0    s_t: pi for a bond; for a ring of N atoms pi exp(-0.025 (N - 14)^2), as published (36.34 degrees for
 *                          N = 6, 23.76 for 5, 14.78 for 4, 180 for 14)
 *   even [T] int32         1 when a reflection leaves the term's value as it is (a ring's tau), 0 when it negates it (a dihedral)
 *   S_p(x -> y) = sum_t w[t] min(1, delta(x[tmap[0][t]], y[tmap[p][t]]) (1 / s_t)) / sum_t w[t],  t ascending, fp64; a term with a
 *   NaN value counts 1.  The cap keeps the value in [0, 1]: a chair (tau = 60 degrees) against a flat ring would otherwise score
 *   1.65 on that term.  out_mirror negates y only where even[t] = 0.  For ring values in [0, pi] delta is the plain |difference|.
 * Both are required.  With every scale pi and every flag 0 the values are agdiff_tfd_matrix's up to the rounding of 1 / pi. */
int agdiff_tfd_matrix_terms(const float* ang_x, const float* ang_y, const int32_t* tmap, const float* w, const float* scale,
                            const int32_t* even, int32_t R, int32_t G, int32_t Q, int32_t T, int32_t P, float thresh, float* out,
                            float* out_mirror, uint64_t* bits, void* stream);

/* ---- geometry validity -----------------------------------------------------------------------------------------------
 * A sampled conformer can be finite and still broken: a bond stretched to 2.5 A, two ring systems pushed through each other, a
 * hydrogen on top of a carbon five bonds away.  Two checks that need the topology only (no force field, no rdkit; the reference
 * has no counterpart).  The host builds their tables (agdiff_amd/validity.py).  No atomics, deterministic bit for bit.
 * Both take d = |p_i - p_j| with every coordinate converted to fp64 before the first subtraction.
 *
 * agdiff_pair_bounds: distances of K named pairs against [lo, hi].
 *   pos [G][n][3]
 *   pairs [K][2] int32, lo [K], hi [K]   atoms of each pair and its bounds in Angstrom (all three may be null when K = 0)
 *   dist [G][K] or null    d as fp32; NaN for a pair that names an atom outside [0, n), which reads nothing
 *   worst [G]              max_k v,  v = (float)max(lo - d, d - hi, 0) on the fp32 d as stored, +inf when that d is not finite;
 *                          0 when K = 0
 *   worst_pair [G] int32   the lowest k attaining worst; -1 when K = 0
 *   n_bad [G] int32        the number of pairs with v > 0
 * One wave per conformer, lanes over the pairs. */
int agdiff_pair_bounds(const float* pos, const int32_t* pairs, const float* lo, const float* hi, int32_t G, int32_t n, int32_t K,
                       float* dist /* [G][K] or null */, float* worst /* [G] */, int32_t* worst_pair /* [G] */,
                       int32_t* n_bad /* [G] */, void* stream);

/* agdiff_clash_scan: every pair i < j of a conformer that is not excluded, against the sum of two radii.
 *   pos [G][n][3], n <= AGDIFF_MAX_ATOMS_LARGE (else AGDIFF_ERR_LIMIT)
 *   radius [n]             > 0 and finite (NOT checked here: the caller does)
 *   ex_ptr [n + 1], ex_idx [ex_ptr[n]] int32   the excluded partners of every atom as a CSR: symmetric, every row strictly
 *                          ascending, entries in [0, n) (NOT checked here: the caller does).  ex_idx may be null when
 *                          ex_ptr[n] = 0.
 *   thresh                 finite and >= 0, else AGDIFF_ERR_ARG
 *   ratio(i, j) = (float)(d / ((double)radius[i] + (double)radius[j])), 0 when d is not finite in fp64
 *   scratch [4 G S] int32  S = ceil(n / AGDIFF_CLASH_SLICE); one partial { bits(min ratio), i, j, count } per (g, slice), written
 *                          by the call
 *   min_ratio [G]          the smallest ratio; +inf when every pair is excluded or n < 2
 *   min_pair [G][2] int32  the lowest (i, j) attaining it, i < j, lowest i first then lowest j; (-1, -1) when there is no pair
 *   n_clash [G] int32      the number of pairs with ratio < thresh, taken on the fp32 ratio
 * Grid (S, G): a workgroup of AGDIFF_CLASH_SLICE threads owns one slice of atoms i of one conformer and walks the atoms j > i in
 * LDS tiles, every lane merging its own ascending exclusion row as j ascends (no n x n mask); a second launch of one wave per
 * conformer reduces the S partials in slice order. */
int agdiff_clash_scan(const float* pos, const float* radius /* [n], > 0 */, const int32_t* ex_ptr, const int32_t* ex_idx,
                      int32_t G, int32_t n, float thresh, int32_t* scratch, float* min_ratio /* [G] */,
                      int32_t* min_pair /* [G][2] */, int32_t* n_clash /* [G] */, void* stream);

/* agdiff_relax_bounds: repair.  The atoms of a conformer that fails the two checks above are moved by small amounts until every
 * bounded distance and every contact of a pair not excluded is back inside the limits those checks test; a conformer that passes
 * them comes back bit for bit.  This is NOT MMFF and no force field: no energies, no torsion terms, no electrostatics -- a
 * projection onto distance bounds from the topology alone (evaluation.py's use_force_field=True still raises).
 *   pos [G][n][3], n <= AGDIFF_RELAX_MAX_ATOMS (else AGDIFF_ERR_LIMIT)
 *   bd_ptr [n + 1], bd_idx / bd_lo / bd_hi [2 K]   every bounded pair once in the row of each of its two atoms (partner, lo, hi),
 *                          within a row in the order of the pair list; b_i = bd_ptr[i + 1] - bd_ptr[i].  The three arrays may be
 *                          null when K = 0.  NOT checked here: the caller does (partners in [0, n), lo <= hi).
 *   radius, ex_ptr, ex_idx exactly what agdiff_clash_scan takes (NOT checked here)
 *   clash                  finite and >= 0;  pad finite and > 0;  omega in (0, 2);  max_iter in [1, AGDIFF_RELAX_MAX_ITERS]:
 *                          else AGDIFF_ERR_ARG, as for a null pointer or pos_out == pos
 * Targets, a little inside the true limits so that the fp32 result passes the checks with room to spare:
 *   bounded entry k:       p_k = min(pad, (hi_k - lo_k) / 2), the interval [lo_k + p_k, hi_k - p_k]
 *   pair (i, j) not excluded: T_ij = clash (r_i + r_j) + pad
 * One iteration from the positions x, all in fp64 (the fp32 coordinates converted first), d = |x_i - x_j|:
 *   u_ij = (x_i - x_j) / d; when d < 1e-9, (1, 0, 0) seen from the lower-indexed atom and (-1, 0, 0) from the other
 *   s_k  = lo_k + p_k - d below the lower target, hi_k - p_k - d above the upper one, else 0  (the signed change of d wanted)
 *   c_ij = max(T_ij - d, 0)
 *   x_i <- x_i + omega / (b_i + 1) [ sum_{k in row i} s_k u_k / 2  +  sum_{j != i not excluded} c_ij u_ij / 2 ]
 * for every atom from the OLD positions (a Jacobi update).  The weight depends on the topology only -- it is not divided by the
 * number of constraints violated at the moment, which jumps when a distance sits exactly on its target, where a projection puts
 * it: with the static weight the map is continuous and a rounding-level difference stays one.
 * Stop rule, evaluated in the same pass as the displacements and before they are applied: done when every |s_k| <= p_k / 2 and
 * every c_ij <= pad / 2.  Otherwise, after max_iter updates the evaluation of the positions they gave is the last one.
 * Before the first iteration the conformer is tested against the true bounds with the exact rules of agdiff_pair_bounds (d as
 * fp32 against lo, hi) and agdiff_clash_scan ((float)(d / (r_i + r_j)) < clash).
 *   pos_out [G][n][3]      must not alias pos
 *   status [G] int32       0 valid as it came, copied through unchanged; 1 repaired: the stop rule was met; 2 max_iter updates
 *                          applied and the stop rule still not met; 3 a coordinate that is not finite, copied through unchanged
 *   iters [G] int32        updates applied (status 2: max_iter)
 *   resid [G]              the largest |s_k| or c_ij the stop rule saw in its last evaluation, in Angstrom; 0 for status 0, +inf for 3
 *   moved [G]              the root mean square over the atoms of |x_final - x_input|, from the fp64 state before the final store
 * One workgroup of 256 threads per conformer, the positions in LDS as fp64 in two buffers; an atom belongs to L lanes (a power of
 * two chosen from n, 1 past 128 atoms where atoms are strided over the threads) whose partial sums meet in a fixed order; each
 * lane merges the atom's ascending exclusion row as j ascends (no n x n mask).  No atomics, deterministic bit for bit; the loop's
 * exit is decided from one LDS value the whole workgroup reads after a barrier. */
int agdiff_relax_bounds(const float* pos, const int32_t* bd_ptr, const int32_t* bd_idx, const float* bd_lo, const float* bd_hi,
                        const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, int32_t G, int32_t n, int32_t K,
                        float clash, float pad, float omega, int32_t max_iter, float* pos_out /* [G][n][3] */,
                        int32_t* status /* [G] */, int32_t* iters /* [G] */, float* resid /* [G] */, float* moved /* [G] */,
                        void* stream);

/* agdiff_relax_planar: agdiff_relax_bounds with one more constraint type, the planes of agdiff_planar_groups' groups (below), in
 * the same launch: a folded aromatic ring, a pyramidal sp2 centre and a twisted double bond are flattened while the bonds are
 * held -- a projection onto a plane shortens them, so this is a superset of agdiff_relax_bounds.  Still NOT MMFF: no energies, no
 * torsion terms, no electrostatics.  It does not choose E or Z either: a double bond twisted past 90 degrees flattens into the
 * other isomer, because nothing here knows which one the molecule is -- unless agdiff_flip_double_bonds (--fix-double-bonds) ran
 * first: it puts every tagged bridge double bond on the right side of 90 degrees, and the flattening then ends in the tagged isomer.
 *   pos ... ex_idx, G, n, K, clash, pad, omega, max_iter, pos_out ... moved   as agdiff_relax_bounds, the same checks
 *   grp_ptr [P + 1], grp_idx   the planar groups as agdiff_planar_groups takes them, 3 .. AGDIFF_PLANAR_MAX_ATOMS members each, P <=
 *                          AGDIFF_FLATTEN_MAX_GROUPS (else AGDIFF_ERR_LIMIT).  NOT checked here: the caller does (members in [0, n))
 *   mb_ptr [n + 1], mb_grp [grp_ptr[P]]   the same memberships by atom: the groups that contain atom i, ascending;
 *                          q_i = mb_ptr[i + 1] - mb_ptr[i].  NOT checked here either
 *                          P = 0: the four tables may be null, and the results are agdiff_relax_bounds'
 *   thresh, flat_to        finite and >= 0, and flat_to + pad <= thresh: else AGDIFF_ERR_ARG, as for P < 0
 * Per group k and iteration, from the positions x in fp64: centroid c_k and unit normal n_k of the best plane exactly as
 * agdiff_planar_groups computes them (one device routine serves both); for a member i the signed distance h = n_k . (x_i - c_k) and
 * the excess e = max(|h| - flat_to, 0): a member already within flat_to of the plane is not moved by that group, so the term is
 * continuous in x like s_k and c_ij.  The update is
 *   x_i <- x_i + omega / (b_i + q_i + 1) [ sum s_k u_k / 2  +  sum c_ij u_ij / 2  -  sum_{groups k with i} sign(h) e n_k ]
 * (the plane term whole: an atom moves alone towards its plane, no partner takes the other half; the sign of n_k cancels).
 * Stop rule: agdiff_relax_bounds' and every e <= pad / 2, so a repaired group has dev <= flat_to + pad / 2 and passes
 * agdiff_planar_groups at thresh with pad / 2 to spare.  Entry test: agdiff_relax_bounds' or (float)dev > thresh for any group,
 * agdiff_planar_groups' own comparison.
 *   status [G] int32       0 valid and flat as it came, copied through unchanged; 1 repaired; 2 max_iter updates applied and the stop
 *                          rule still not met; 3 a coordinate that is not finite, copied through unchanged
 *   resid [G]              the largest |s_k|, c_ij or e of the last evaluation; iters and moved as agdiff_relax_bounds
 * agdiff_relax_bounds' kernel with two phases per iteration: thread k computes the plane of group k into LDS (six fp64), a barrier,
 * then the atom loop with the plane terms of the atom's membership row.  No atomics, deterministic bit for bit. */
int agdiff_relax_planar(const float* pos, const int32_t* bd_ptr, const int32_t* bd_idx, const float* bd_lo, const float* bd_hi,
                        const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, const int32_t* grp_ptr /* [P + 1] */,
                        const int32_t* grp_idx, const int32_t* mb_ptr /* [n + 1] */, const int32_t* mb_grp, int32_t G, int32_t n,
                        int32_t K, int32_t P, float clash, float pad, float omega, int32_t max_iter, float thresh, float flat_to,
                        float* pos_out /* [G][n][3] */, int32_t* status /* [G] */, int32_t* iters /* [G] */, float* resid /* [G] */,
                        float* moved /* [G] */, void* stream);

/* agdiff_planar_groups: planarity.  Bent aromatic rings, pyramidal sp2 centres and twisted double bonds keep every distance the
 * checks above test legal; this one measures, for P named groups of atoms that should lie in one plane (the host names them from
 * the bond types: agdiff_amd/planarity.py), how far the members are from the group's best plane.
 *   pos [G][n][3]
 *   grp_ptr [P + 1], grp_idx [grp_ptr[P]] int32   the members of every group as a CSR (both may be null when P = 0).  grp_ptr is
 *                          NOT checked here: the caller does (starts at 0, does not decrease, ends at the length of grp_idx)
 *   thresh                 finite and >= 0, else AGDIFF_ERR_ARG
 * Per (conformer, group) of m members, in fp64 from the fp32 coordinates: centroid c, y_k = x_k - c, A = (1 / m) sum_k y_k y_k^T,
 * unit normal = the eigenvector of A's smallest eigenvalue (cyclic Jacobi sweeps, the solver of the RMSD kernels),
 *   dev [G][P] or null     (float)max_k |normal . y_k|: the largest distance of a member from the best plane, in Angstrom; +inf when a
 *                          member coordinate is not finite; NaN for a group of fewer than 3 or more than AGDIFF_PLANAR_MAX_ATOMS
 *                          members or one that names an atom outside [0, n): such a group reads no coordinate and enters neither
 *                          worst nor n_bent
 *   worst [G]              the maximum of the fp32 dev values as stored; 0 when P = 0 or every group is NaN
 *   worst_group [G] int32  the lowest group index attaining worst; -1 when P = 0 or every group is NaN
 *   n_bent [G] int32       the number of groups with dev > thresh (+inf counts)
 * dev is defined through the projections and not as sqrt(lambda_min): on an exactly planar group the eigenvalue is rounding noise
 * of A (sqrt of 1e-15 is 3e-8 A) while the projections on the computed normal are not.
 * One wave per conformer, lanes over the groups.  No atomics, deterministic bit for bit. */
int agdiff_planar_groups(const float* pos, const int32_t* grp_ptr /* [P + 1] */, const int32_t* grp_idx, int32_t G, int32_t n, int32_t P,
                         float thresh, float* dev /* [G][P] or null */, float* worst /* [G] */, int32_t* worst_group /* [G] */,
                         int32_t* n_bent /* [G] */, void* stream);

/* ---- trajectory tracking ---------------------------------------------------------------------------------------------
 * The convergence curve of examples/test_alanine_dipeptide.py:106-164 (every frame of the denoising run superposed on a target
 * structure, heavy-atom RMSD) for a PACKED batch, without keeping the trajectory: epsnet.LangevinRun calls this once per NaN
 * poll over the frames written since the last one (agdiff_amd/trajectory.py).
 *
 * agdiff_traj_rmsd: out[s][g] = RMSD of graph g in frame s to the same atoms of `target` after the optimal proper rotation +
 * translation, over the graph's atoms with select != 0, identity atom mapping (no symmetry: what mdtraj's rmsd does).
 *   frames                 S frames of a packed batch, [N][3] each, frame s at frames + s * frame_stride (in floats,
 *                          >= 3 N, else AGDIFF_ERR_ARG): a trajectory, a ring of frames or a strided view of either
 *   target [N][3]          packed like a frame; need not be centred
 *   select [N] uint8       1 = the atom enters
 *   graph_ptr [G + 1]      first atom of every graph (agdiff_topo_t.graph_ptr); entries are clamped to [0, N]
 *   out [S][G]             sqrt(max((|X|^2 + |Y|^2 - 2 lambda_max(K)) / m, 0)), m = the graph's selected atoms: centroids in
 *                          fp64, centred coordinates rounded to fp32 once, cross-covariance and norms in fp64 from those
 *                          (the arithmetic of agdiff_rmsd_matrix with another summation order: equal to ~1e-7, not bit for bit)
 *   out_mirror [S][G] or null   sqrt(max((|X|^2 + |Y|^2 + 2 lambda_min(K)) / m, 0)): the RMSD of the frame's mirror image, from the
 *                          same diagonalisation.  Not overlapping out.
 * Both are NaN for an (s, g) in which a selected coordinate of the frame or of the target is not finite (no other entry
 * changes), and for a graph without a selected atom.  One 64-lane wave per (g, s), lanes striding over the graph's atoms: any
 * number of atoms per graph.  No atomics, deterministic bit for bit, independent of S and of frame_stride. */
int agdiff_traj_rmsd(const float* frames, int64_t frame_stride /* floats between frames, >= 3 N */,
                     const float* target /* [N][3] */, const uint8_t* select /* [N] */, const int32_t* graph_ptr /* [G + 1] */,
                     int32_t S, int32_t G, int32_t N, float* out /* [S][G] */, float* out_mirror /* [S][G] or null */,
                     void* stream);

/* ---- rigid core hold ------------------------------------------------------------------------------------------------------
 * Conformers around a fixed core (what rdkit's coordMap / ConstrainedEmbed are used for): epsnet.LangevinRun calls this after a
 * step's update, so that the selected atoms of every graph keep the INTERNAL geometry of a template while the core floats rigidly
 * with the rest of the molecule (the score network sees distances only).
 *
 * agdiff_hold_core: for graph g with selected atoms A (m = |A|), in place:
 *   fit_a  = R (t_a - c_t) + c_x     c_x, c_t the centroids of pos[A] and core_pos[A]; R the proper rotation (Horn's quaternion of
 *                                    lambda_max of the cross-covariance, cyclic Jacobi) that takes the centred template onto the
 *                                    centred current core; all of it in fp64 from the stored fp32 coordinates
 *   pos[a] = pos[a] + weight (fit_a - pos[a]) for a in A, rounded to fp32 once; weight == 1 stores fit_a itself.  Atoms outside
 *            A are not written: they keep their bits.
 *   pos [N][3]             a packed batch, read and written
 *   core_pos [N][3]        the template, packed like pos; need not be centred; only the selected rows are read
 *   select [N] uint8       1 = the atom belongs to the core
 *   graph_ptr [G + 1]      first atom of every graph (agdiff_topo_t.graph_ptr); entries are clamped to [0, N]
 *   skip [G] int32 or null != 0: the graph is left alone (agdiff_ws_t.nan_flag + 1: a quarantined graph holds a placeholder)
 *   weight                 in (0, 1], else AGDIFF_ERR_ARG
 *   copy_out [N][3] or null  the values written to pos[a], a in A, go to copy_out[a] too (the trajectory row the update kernel has
 *                          just written); no other entry is touched.  Not pos, not core_pos.
 *   dev [G] or null        sqrt(max((sum |x - c_x|^2 + sum |t - c_t|^2 - 2 lambda_max) / m, 0)): the RMSD over A between the core
 *                          BEFORE this call and the fit -- how far the step before pulled the core out of shape
 * A graph is left untouched, with dev[g] = NaN, when it has no selected atom, when skip[g] != 0, or when a selected coordinate of
 * pos or of core_pos is not finite.  Any m >= 1: m = 1 leaves the atom where it is; where the rotation is not unique (m = 2,
 * collinear atoms) one maximiser is taken, as by agdiff_align_conformers.  Proper rotations only: a template is held in ITS
 * handedness.  Identity atom mapping.  One 64-lane wave per graph, lanes striding over the graph's atoms: any number of atoms
 * per graph.  Every read that feeds the sums is reduced across the wave before the first store.  No atomics, deterministic bit
 * for bit. */
int agdiff_hold_core(float* pos /* [N][3], in place */, const float* core_pos /* [N][3] */, const uint8_t* select /* [N] */,
                     const int32_t* graph_ptr /* [G + 1] */, const int32_t* skip /* [G] or null: != 0 leaves the graph alone */,
                     int32_t G, int32_t N, float weight /* (0, 1] */, float* copy_out /* [N][3] or null */,
                     float* dev /* [G] or null */, void* stream);

/* ---- distance restraints ---------------------------------------------------------------------------------------------------
 * Conformers under distance restraints (a macrocycle or staple closure, an NOE contact, a pharmacophore distance, a lower bound
 * that keeps the ensemble extended): epsnet.LangevinRun calls this after a step's update, before agdiff_hold_core when a core is
 * held too, so that the network relaxes the rest of the molecule around the restraint (agdiff_amd/restraints.py).
 *
 * agdiff_restrain_pairs: flat-bottomed windows [lo, hi] on interatomic distances of a packed batch, in place.
 *   pos [N][3]             a packed batch, read and written
 *   graph_ptr [G + 1]      first atom of every graph (agdiff_topo_t.graph_ptr); entries are clamped to [0, N]
 *   rs_ptr [N + 1], rs_idx [R2], rs_lo [R2], rs_hi [R2]
 *                          the by-atom table over the batch's atoms, exactly validity.bounds_csr(N, pairs, lo, hi) with batch-level
 *                          atom indices (R2 = 2 R entries for R pairs): row a = rs_ptr[a] .. rs_ptr[a + 1] lists (partner b, lo, hi)
 *                          for every pair of atom a, every pair once in the row of each of its two atoms, rows in the order of the
 *                          pair list; a pair listed twice counts twice.  The HOST checks 0 <= lo <= hi (hi may be +inf: a lower
 *                          bound only), no NaN, a != b, both atoms in the same graph; here a partner outside the graph's atoms is
 *                          skipped unread and row bounds are clamped to [0, R2].  rs_idx / rs_lo / rs_hi may be null for R2 == 0.
 *   fixed [N] uint8 or null   1 = the atom is not moved by a sweep (a held core's atoms); its partners take the whole step
 *   skip [G] int32 or null != 0: the graph is left alone (agdiff_ws_t.nan_flag + 1)
 *   max_restrained         the largest number of atoms with a row in one graph of the batch, <= AGDIFF_RESTRAIN_MAX_ATOMS (else
 *                          AGDIFF_ERR_LIMIT, before any launch); a graph that has more all the same is left alone, viol = NaN
 *   weight w               in (0, 1], else AGDIFF_ERR_ARG
 *   sweeps                 in [0, 16], else AGDIFF_ERR_ARG; 0 moves nothing and only measures
 *   copy_out [N][3] or null  the values of the last sweep written to pos[a], for the atoms with a row, go to copy_out[a] too (the
 *                          trajectory frame); no other entry is touched; untouched when sweeps == 0.  Not pos.
 *   viol [G] or null       the largest |e| over the graph's rows BEFORE the first sweep; 0 for a graph without restraints
 * One sweep, for atom a with a row of length c_a > 0, all positions read as they were before the sweep (Jacobi), in fp64 from the
 * stored fp32.  For each row entry (b, lo, hi):
 *   d = |x_a - x_b|;   e = d - hi if d > hi, d - lo if d < lo, else 0
 *   s = 0 if fixed[a], 1 if fixed[b], else 1/2 (the share of atom a)
 *   an entry with d < 1e-12 or d not finite moves nothing in that sweep
 * then x_a <- x_a + (w / c_a) sum s (-e) (x_a - x_b) / d, rounded to fp32 once per sweep; an atom none of whose entries
 * contributes keeps its bits.  The division by the STATIC row length c_a keeps the rule continuous in the positions and stable for
 * an atom with many restraints for any w in (0, 1]; a single pair with w = 1 and both ends free lands exactly on its violated
 * bound and keeps the pair's centroid (a sweep with a fixed end moves it).  Atoms with an empty row are not written; atoms of a
 * graph whose restraints are all satisfied keep their bytes.  Positions pass through fp32 between sweeps: that rounding is part of
 * the rule.  A graph with skip[g] != 0, or with a restrained atom (or partner) whose coordinate is not finite, is not written at all
 * and gets viol[g] = NaN.  One 64-lane wave per graph, lanes striding over the graph's atoms and gathering their own rows: any
 * number of atoms per graph.  A sweep's new values wait in LDS until every read of the sweep is done.  No atomics, deterministic bit
 * for bit. */
int agdiff_restrain_pairs(float* pos /* [N][3], in place */, const int32_t* graph_ptr /* [G + 1] */, const int32_t* rs_ptr /* [N + 1] */,
                          const int32_t* rs_idx /* [R2] */, const float* rs_lo /* [R2] */, const float* rs_hi /* [R2] */,
                          const uint8_t* fixed /* [N] or null */, const int32_t* skip /* [G] or null: != 0 leaves the graph alone */,
                          int32_t G, int32_t N, int32_t R2, int32_t max_restrained, float weight /* (0, 1] */,
                          int32_t sweeps /* [0, 16] */, float* copy_out /* [N][3] or null */, float* viol /* [G] or null */,
                          void* stream);

/* ---- torsion restraints ----------------------------------------------------------------------------------------------------
 * Conformers under torsion restraints (a torsion scan, a fixed phi / psi pair, an amide held trans, a biaryl twist held to a
 * docking pose -- what a distance window cannot say: a 1-4 distance fixes |theta| at best, never its sign): epsnet.LangevinRun
 * calls this after a step's update, after agdiff_restrain_pairs and before agdiff_hold_core
 * (agdiff_amd/torsion_restraints.py).
 *
 * agdiff_restrain_torsions: circular windows centre +- half on dihedrals of a packed batch, in place.
 *   pos [N][3]             a packed batch, read and written
 *   graph_ptr [G + 1]      first atom of every graph (agdiff_topo_t.graph_ptr); entries are clamped to [0, N]
 *   tr_ptr [G + 1]         the restraints of graph g are rows tr_ptr[g] .. tr_ptr[g + 1] of the four arrays below, walked in
 *                          row order; entries are clamped to [0, T]
 *   quads [T][4]           batch-level atoms (a, u, v, b): theta = atan2(|b2| b1 . n2, n1 . n2), b1 = p_u - p_a, b2 = p_v - p_u,
 *                          b3 = p_b - p_v, n1 = b1 x b2, n2 = b2 x b3, agdiff_torsion_angles' formula in fp64 from the stored fp32
 *   centre [T], half [T]   the window in radians, |centre| <= pi and half in [0, pi] (the HOST checks); half = pi: always satisfied
 *   side_row [T]           row of the side table whose atoms the restraint turns, -1 (or anything outside [0, S)): measure only
 *   side_ptr [S + 1], side_idx   the side table: row r = side_ptr[r] .. side_ptr[r + 1] lists OFFSETS FROM THE GRAPH'S FIRST ATOM,
 *                          so all conformers of a molecule share one row.  A row always lists atoms that turn with the v, b end
 *                          of its quad (the host reverses a quad whose smaller side is u's: theta(a, u, v, b) = theta(b, v, u, a)).
 *                          An offset outside the graph, or one naming u or v (they lie on the axis), is skipped, and so is a listed
 *                          atom with a coordinate that is not finite: each stays bit for bit.  May be null for S == 0.
 *   skip [G] int32 or null != 0: the graph is left alone (agdiff_ws_t.nan_flag + 1)
 *   weight w               in (0, 1], else AGDIFF_ERR_ARG
 *   turn                   0: only measure, nothing is written to pos or copy_out
 *   copy_out [N][3] or null  receives every value stored to pos and nothing else (the trajectory frame).  Not pos.
 *   angle [T] or null      theta as found when the restraint's turn comes (turn == 0: as it is), NaN for a degenerate quad -- a
 *                          zero normal, or an atom outside its graph, in which case it reads nothing -- which is not turned and does
 *                          not enter viol; NaN for every restraint of a graph that is left alone
 *   viol [G]               the largest |e| in radians over the graph's restraints BEFORE the call, 0 without restraints
 * The excess: Delta = theta - centre wrapped into [-pi, pi]; |Delta| <= half: satisfied, nothing of the restraint is written;
 * else e = Delta - sign(Delta) half.  The window is circular: centre 170 degrees with half 20 degrees contains -175 degrees.
 * A restraint with e != 0, turn != 0 and a non-empty side row turns every listed atom by phi = -w e about the axis through p_v
 * along k = (p_v - p_u) / |p_v - p_u|, right-handed: r' = r cos phi + (k x r) sin phi + k (k . r) (1 - cos phi), r = p - p_v, in
 * fp64, rounded to fp32 once.  Turning that side by +phi changes theta by +phi, so theta' = theta - w e, and w = 1 lands on the
 * violated edge of the window.  The rotation is proper and rigid: every distance within either side and every tetrahedral parity
 * is kept.  A rigid turn about a bridge leaves every dihedral about another bond unchanged, so restraints on distinct bridges
 * are independent and one pass at w = 1 satisfies all of them.
 * A measure pass over the graph's restraints comes before anything is written.  A graph with skip[g] != 0, or with a quad
 * coordinate that is not finite, is not written at all and gets viol[g] = NaN.  One 64-lane wave per graph walks the restraints in
 * row order, lanes striding over the side row, with a workgroup barrier after each rotation: any number of atoms and of
 * restraints, no LDS.  No atomics, deterministic bit for bit. */
int agdiff_restrain_torsions(float* pos /* [N][3], in place */, const int32_t* graph_ptr /* [G + 1] */,
                             const int32_t* tr_ptr /* [G + 1]: the restraints of graph g are rows tr_ptr[g] .. tr_ptr[g + 1] */,
                             const int32_t* quads /* [T][4] batch-level atoms (a, u, v, b) */,
                             const float* centre /* [T] rad */, const float* half /* [T] rad, in [0, pi] */,
                             const int32_t* side_row /* [T]: row of the side table, -1 = measure only */,
                             const int32_t* side_ptr /* [S + 1] */, const int32_t* side_idx /* offsets from the graph's first atom */,
                             const int32_t* skip /* [G] or NULL */, int32_t G, int32_t N, int32_t T, int32_t S,
                             float weight, int32_t turn /* 0: only measure */, float* copy_out /* [N][3] or NULL */,
                             float* angle /* [T] or NULL */, float* viol /* [G] */, void* stream);

/* ---- distance-distribution MMD -----------------------------------------------------------------------------------------
 * The maximum mean discrepancy between the interatomic-distance distributions of the generated and the reference conformers of
 * one molecule, as the ConfGF / CGCF / GraphDG line reports it ("all", and "single" per atom pair; their "pair" mode, over all
 * pairs of columns, is not built).  The tables are what agdiff_pair_bounds writes as `dist`.
 *   tab_x [R][K], tab_y [G][K]   fp32 distances of K atom pairs in the R reference and the G generated conformers
 *   Z = [X; Y], M = R + G, R >= 1, G >= 1, K >= 1; all arithmetic in fp64 from the stored fp32 values
 *   D2(a, b)  = sum_k (Z[a][k] - Z[b][k])^2
 *   b         = sum_{a, b} D2(a, b) / (M^2 - M), computed as the equal 2 M sum_a |Z[a] - mu|^2 / (M^2 - M), mu the column mean
 *   k(a, b)   = sum_{i = 0 .. 4} exp(-D2(a, b) / (b 2^(i - 2)));  k(a, a) = 5, and the diagonal is included (biased V-statistic)
 *   mmd2      = mean_{a, b in X} k + mean_{a, b in Y} k - 2 mean_{a in X, b in Y} k, stored as fp32
 *   b == 0 (all rows equal): mmd2 = 0.  An entry that is not finite in the rows / columns involved: mmd2 = bandwidth = NaN.
 *
 * agdiff_mmd_all: ONE problem over the K-dimensional rows.
 *   scratch   8-byte aligned, 8 (K + 1 + 3 T (T + 1) / 2) bytes, T = ceil(M / 16); written by the call
 *   mmd2 [1], bandwidth [1]   (bandwidth = b as fp32)
 *   T (T + 1) / 2 >= 2^24 tiles (M > 92,672): AGDIFF_ERR_LIMIT -- the grid of 256-thread workgroups stays below 2^32 threads
 * A statistics pass (column means and scatters, 16 columns per workgroup), one wave that sums the scatters into b, one workgroup
 * per 16 x 16 tile of the upper triangle of the M x M pairs (off-diagonal pairs weighted twice, table rows staged in LDS 64
 * columns at a time, one exponential and four squarings per pair, one partial { XX, YY, XY } per tile) and one wave that sums the
 * partials in tile order.
 *
 * agdiff_mmd_single: K independent one-dimensional problems, column k of both tables each.
 *   scratch   8-byte aligned, 16 K + 4 K M bytes; written by the call (the column scatters, the fp64 bandwidths and the table
 *             transposed to [K][M]: the statistics pass transposes, the callers pass [R][K] / [G][K] as to agdiff_mmd_all)
 *   mmd2 [K], bandwidth [K]   a column with an entry that is not finite is NaN in both; no other column changes
 *   M > AGDIFF_MMD_MAX_CONFS: AGDIFF_ERR_LIMIT
 * The statistics pass, then one workgroup of 1024 threads per column: its M values in LDS, the pairs a <= b numbered row by row
 * and dealt to the threads round robin.
 * Both: AGDIFF_ERR_ARG for R < 1, G < 1, K < 1 or a null pointer.  No atomics, deterministic bit for bit; multiplying both tables
 * by a power of two changes no bit of mmd2. */
int agdiff_mmd_all(const float* tab_x /* [R][K] */, const float* tab_y /* [G][K] */, int32_t R, int32_t G, int32_t K, void* scratch,
                   float* mmd2 /* [1] */, float* bandwidth /* [1] */, void* stream);
int agdiff_mmd_single(const float* tab_x /* [R][K] */, const float* tab_y /* [G][K] */, int32_t R, int32_t G, int32_t K, void* scratch,
                      float* mmd2 /* [K] */, float* bandwidth /* [K] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AGDIFF_HIP_H */
