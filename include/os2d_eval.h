/* C ABI of libos2d_eval.so: the PASCAL VOC detection metric (mAP, recall) of a whole dataset on the device (gfx950).
 *
 * Every pointer is a device pointer unless said otherwise, `stream` is a hipStream_t, every call only enqueues work.
 * Return value: 0, or a negative code with the text in os2d_eval_last_error() (-1 bad argument, -2 workspace too small,
 * -4 launch failure).  Plain indices are 32-bit (D < 2^31 detections); the winner word of the match step is 64-bit.
 *
 * Packing: detections of image n are rows det_offsets[n] .. det_offsets[n+1]-1 of boxes[D][4] (xmin, ymin, xmax, ymax, fp32),
 * scores[D] (fp32), labels[D] (int32); ground truth likewise with gt_offsets[N+1], gt_labels[G] (int32) and
 * gt_difficult[G] (uint8).  Labels lie in [0, L).
 *
 * Labels outside [0, L) are tolerated, not validated (that would need a synchronisation): such a ground-truth box is not
 * counted; such a detection is filed BEHIND every class in the per-class ordering, so the numbers of the classes 0 .. L-1
 * are those of the same call without it, and it stays in the joint ordering.  The match step has no L and only compares
 * labels: such a detection can match only a ground-truth box of the same out-of-range label (which count_gt did not
 * count); with ground-truth labels in range it matches nothing (match 0) and is a false positive of the joint class.
 * Boxes whose area under the +1 convention is not positive (xmax + 1 <= xmin) give a NaN or negative IoU and are outside
 * the contract.
 */
#ifndef OS2D_EVAL_H
#define OS2D_EVAL_H
#include <stddef.h>

#define OS2D_EVAL_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int os2d_eval_abi_version(void);
const char* os2d_eval_last_error(void);

/* n_pos[L+1]: ground-truth boxes per label that are not difficult, slot L their total; gt_count[L]: all boxes per label.
 * Both are zeroed here. */
int os2d_eval_count_gt(const int* gt_labels, const unsigned char* gt_difficult, int G, int L, int* n_pos, int* gt_count,
                       void* stream);

/* match[D] (int8): 1 = the best-scoring detection assigned to a ground-truth box, 0 = a later one or one without a box,
 * -1 = assigned to a difficult box.  gt_index[D] (int32) and winner[G] (uint64) are workspace. */
int os2d_eval_match(const float* det_boxes, const float* det_scores, const int* det_labels, const int* det_offsets, int D, int N,
                    const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult, const int* gt_offsets, int G,
                    float iou_thresh, int* gt_index, unsigned long long* winner, signed char* match, void* stream);

/* Stable sorts of the detection indices: perm_joint[D] by descending score, perm_class[D] by (label, descending score);
 * ties keep increasing index.  sorted_labels[D] = labels[perm_class], class_offsets[L+1] = first position of every label in
 * it.  label_bits: bits needed for L - 1; more are allowed and change nothing.  A detection whose label is outside [0, L)
 * is sorted with the key L: those rows are the positions class_offsets[L] .. D-1 of perm_class, in descending score, and
 * sorted_labels holds L there (so class_offsets[L] is the number of detections with a label in range).  D = 0 zeroes
 * class_offsets and touches nothing else.  The workspace holds nothing the caller may rely on afterwards. */
size_t os2d_eval_sort_workspace_bytes(int D);
int os2d_eval_sort(const float* det_scores, const int* det_labels, int D, int L, int label_bits, unsigned int* perm_joint,
                   unsigned int* perm_class, int* sorted_labels, int* class_offsets, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Precision / recall curves of one ordering.  seg: the label of every position (sorted_labels), non-decreasing, any int
 * (a label outside [0, L), -1 included, has n_pos 0 and no rec_last / acc entry), or NULL for one segment of all D
 * positions; n_pos / rec_last are indexed by that label (index 0 when seg is NULL).  tpfp[D] (uint64, tp in the high word)
 * may be NULL.  rec_last[s] receives the last recall of a segment; entries of segments without positions are left. */
size_t os2d_eval_scan_workspace_bytes(int D);
int os2d_eval_prec_rec(const signed char* match, const unsigned int* perm, const int* seg, const int* n_pos, int L, int D,
                       unsigned long long* tpfp, double* prec, double* rec, double* rec_last, void* workspace,
                       size_t workspace_bytes, void* stream);

/* mpre[D]: the running maximum of nan_to_num(prec) from every position to the end of its segment.  acc[s * 11 + t]:
 * use_07_metric = 0: t = 0 receives the area under the curve of segment s; = 1: the 11 interpolated precisions.  acc is
 * zeroed by the caller (a segment without detections writes nothing). */
int os2d_eval_ap(const double* prec, const double* rec, const int* seg, int L, int D, int use_07_metric, double* mpre, double* acc,
                 void* workspace, size_t workspace_bytes, void* stream);

/* acc[(L+1) * 11], rec_last[L+1], n_pos[L+1]: slots 0 .. L-1 per class, slot L the joint class.  Writes ap_per_class[L],
 * recall_per_class[L], n_pos_out[L] (fp64) and scalars[4] = map, map_weighted, recall, ap_joint_classes. */
int os2d_eval_finalise(const double* acc, const double* rec_last, const int* n_pos, int L, int use_07_metric, double* ap_per_class,
                       double* recall_per_class, double* n_pos_out, double* scalars, void* stream);

#ifdef __cplusplus
}
#endif
#endif
