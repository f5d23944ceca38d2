"""References for PointRCNN's target assignment (include/dfu3d_tgt.h) and its losses.  Importable without the reference
and without a GPU.

1. Sequential NumPy restatements of the three kernels, one float32 (where the header says so, float64) operation per
   element in the order of the header's expressions, trig and log evaluated in float64 and rounded once:
   point_targets, max_iou (over an IoU matrix the caller supplies: the footprint overlap has its own tests) and subsample.
2. A plain-torch formulation of the targets in the reference's own shape -- per-sample loops, boolean indexing, host reads
   -- on whatever device its inputs are on: plain_point_targets, plain_max_iou, plain_subsample, plain_proposal_targets,
   plain_roi_targets.
3. Both heads' losses from their formulas on torch primitives alone (plain_point_losses, plain_rcnn_losses): they import
   nothing of the package's loss functions, corner helper or box coders, so they check them."""
import math

import numpy as np

from tests import roipoint_ref as R

F32, F64 = np.float32, np.float64
MIN_DIM = F32(1e-5)


# ---- 1. the restatements ----------------------------------------------------------------------------------------------
def encode_point(box, pt, mean):
    """box float32 (8), pt float32 (3), mean float32 (3) or None -> the eight code columns (float32)."""
    with np.errstate(all='ignore'):
        d = [MIN_DIM if v < MIN_DIM else v for v in box[3:6]]
        if mean is not None:
            diag = np.sqrt(mean[0] * mean[0] + mean[1] * mean[1])
            head = [(box[0] - pt[0]) / diag, (box[1] - pt[1]) / diag, (box[2] - pt[2]) / mean[2]]
            dims = [F32(np.log(F64(d[k] / mean[k]))) for k in range(3)]
        else:
            head = [box[0] - pt[0], box[1] - pt[1], box[2] - pt[2]]
            dims = [F32(np.log(F64(d[k]))) for k in range(3)]
        return np.array(head + dims + [F32(np.cos(F64(box[6]))), F32(np.sin(F64(box[6])))], F32)


def point_targets(points, gt_boxes, extra, num_class, mean_size=None):
    """points float32 (B, N, 3), gt_boxes float32 (B, G, 8), mean_size (K, 3) or None -> cls int64 (B * N), box float32
    (B * N, 8), gt_idx int32 (B * N)."""
    points, gt = np.asarray(points, F32), np.asarray(gt_boxes, F32)
    mean = None if mean_size is None else np.asarray(mean_size, F32)
    B, N = points.shape[:2]
    G = gt.shape[1]
    cls, box, idx = np.zeros(B * N, np.int64), np.zeros((B * N, 8), F32), np.full(B * N, -1, np.int32)
    zero = (0.0, 0.0, 0.0)
    for b in range(B):
        inside = np.stack([R.in_box(R.load_box(gt[b, g, :7], zero), points[b]) for g in range(G)])        # (G, N)
        around = np.stack([R.in_box(R.load_box(gt[b, g, :7], extra), points[b]) for g in range(G)])
        for n in range(N):
            k = int(np.argmax(inside[:, n])) if inside[:, n].any() else -1
            e = int(np.argmax(around[:, n])) if around[:, n].any() else -1
            row = b * N + n
            idx[row] = k
            if k >= 0:
                c = gt[b, k, 7]
                if c >= 1 and c < 2147483648.0 and (mean is None or c <= len(mean)):
                    cls[row] = 1 if num_class == 1 else int(c)
                    box[row] = encode_point(gt[b, k], points[b, n], None if mean is None else mean[int(c) - 1])
            elif e >= 0:
                cls[row] = -1
    return cls, box, idx


def row_sum(row):
    s = F32(row[0])
    with np.errstate(all='ignore'):
        for v in row[1:]:
            s = F32(s + F32(v))
    return s


def max_iou(iou, roi_labels, gt_boxes, by_class):
    """iou float32 (B, M, G): the IoU of every RoI with every row; roi_labels int (B, M); gt_boxes float32 (B, G, 8) ->
    max_overlaps float32 (B, M), gt_assignment int32 (B, M) by the header's eligibility, tie and NaN rules."""
    iou, gt = np.asarray(iou, F32), np.asarray(gt_boxes, F32)
    B, M, G = iou.shape
    ov, asg = np.zeros((B, M), F32), np.zeros((B, M), np.int32)
    for b in range(B):
        last = max([g for g in range(G) if row_sum(gt[b, g]) != 0] + [-1])
        for m in range(M):
            best, best_g = F32(0), -1
            for g in range(last + 1):
                if by_class:
                    c = gt[b, g, 7]
                    if not (abs(c) < 9.0e18) or int(c) != int(roi_labels[b, m]):
                        continue
                v = iou[b, m, g]
                if v == v and (best_g < 0 or v > best):
                    best, best_g = v, g
            if best_g >= 0:
                ov[b, m], asg[b, m] = best, best_g
    return ov, asg


def sampler_numbers(cfg):
    R_ = int(cfg['ROI_PER_IMAGE'])
    return (R_, int(np.round(cfg['FG_RATIO'] * R_)), F32(min(cfg['REG_FG_THRESH'], cfg['CLS_FG_THRESH'])),
            F32(cfg['REG_FG_THRESH']), F32(cfg['CLS_BG_THRESH_LO']), float(cfg['HARD_BG_RATIO']))


def draw(lst, u):
    n = len(lst)
    v = math.floor(float(F64(u) * n)) if u == u else -1
    return lst[(int(v) if v < n else n - 1) if v >= 0 else 0]


def lists_of(ov, cfg):
    """One sample's max_overlaps -> (fg, hard, easy) index lists in ascending order."""
    _, _, fg_t, reg_t, lo_t, _ = sampler_numbers(cfg)
    ov = np.asarray(ov, F32)
    with np.errstate(all='ignore'):
        return ([i for i in range(len(ov)) if ov[i] >= fg_t], [i for i in range(len(ov)) if ov[i] < reg_t and ov[i] >= lo_t],
                [i for i in range(len(ov)) if ov[i] < lo_t])


def subsample(max_overlaps, cfg, rand_key, rand_u):
    """max_overlaps float32 (B, M), rand_key int32 (B, M), rand_u float32 (B, R) -> sampled_inds int32 (B, R), status,
    parts: per sample (take, h, source of the background slots) for the tests' branch table."""
    ov, key, u = np.asarray(max_overlaps, F32), np.asarray(rand_key, np.int32), np.asarray(rand_u, F32)
    R_, fg_per, _, _, _, ratio = sampler_numbers(cfg)
    B = ov.shape[0]
    out, status, parts = np.zeros((B, R_), np.int32), 0, []
    for b in range(B):
        fg, hard, easy = lists_of(ov[b], cfg)
        nf, nh, ne = len(fg), len(hard), len(easy)
        if nf == 0 and nh + ne == 0:
            status |= 1
            parts.append(('none', 0, 0))
            continue
        if nh + ne == 0:
            out[b] = [draw(fg, u[b, j]) for j in range(R_)]
            parts.append(('fg_only', 0, 0))
            continue
        take = 0
        if nf > 0:
            take = min(fg_per, nf)
            order = sorted(range(nf), key=lambda t: (int(key[b, fg[t]]), t))
            out[b, :take] = [fg[t] for t in order[:take]]
        need = R_ - take
        h = min(int(float(need) * ratio), nh) if (nh > 0 and ne > 0) else (need if nh > 0 else 0)
        for j in range(take, R_):
            out[b, j] = draw(hard, u[b, j]) if j - take < h else draw(easy, u[b, j])
        parts.append(('both' if nf > 0 else 'bg_only', take, h))
    return out, status, parts


# ---- 2. the plain formulation -------------------------------------------------------------------------------------------
def torch_points_in_boxes(points, boxes7, margin=1e-5):
    """points (N, 3), boxes7 (G, 7) -> int64 (N): the first box that holds the point, -1 for none; the in-box test of
    csrc/pt_in_box.hpp in torch (float32 rotation, float64 comparisons)."""
    import torch
    cosa, sina = torch.cos(-boxes7[:, 6].double()).float(), torch.sin(-boxes7[:, 6].double()).float()
    sx, sy = points[:, None, 0] - boxes7[None, :, 0], points[:, None, 1] - boxes7[None, :, 1]
    lx, ly = sx * cosa + sy * (-sina), sx * sina + sy * cosa
    hz, hx, hy = boxes7[:, 5].double() / 2.0, boxes7[:, 3].double() / 2.0 + float(F32(margin)), boxes7[:, 4].double() / 2.0 + float(F32(margin))
    inside = (~((points[:, None, 2] - boxes7[None, :, 2]).abs().double() > hz) & (lx.abs().double() < hx) & (ly.abs().double() < hy))
    first = torch.argmax(inside.long(), dim=1)
    return torch.where(inside.any(dim=1), first, torch.full_like(first, -1))


def plain_point_targets(point_coords, gt_boxes, extra, num_class, coder):
    """PointHeadTemplate.assign_stack_targets with set_ignore_flag and ret_box_labels, in its own shape: per sample a
    mask, two point-in-box searches, boolean-indexed scatters and an encode of the foreground subset.  Rows of class < 1
    are left background (this package's recorded divergence).  gt_boxes is not written."""
    import torch
    from dfu3d_amd.pcdet_kitti import box_utils
    B = gt_boxes.shape[0]
    large = box_utils.enlarge_box3d(gt_boxes.view(-1, gt_boxes.shape[-1]), extra_width=extra).view(B, -1, gt_boxes.shape[-1])
    bs_idx = point_coords[:, 0]
    cls = point_coords.new_zeros(point_coords.shape[0]).long()
    box = gt_boxes.new_zeros((point_coords.shape[0], 8))
    for k in range(B):
        mask = bs_idx == k
        pts = point_coords[mask][:, 1:4]
        cls_one = cls.new_zeros(int(mask.sum()))
        idx = torch_points_in_boxes(pts, gt_boxes[k, :, 0:7])
        fg = idx >= 0
        ignore = fg ^ (torch_points_in_boxes(pts, large[k, :, 0:7]) >= 0)
        cls_one[ignore] = -1
        rows = gt_boxes[k][idx.clamp(min=0)]
        fg = fg & (rows[:, -1] >= 1)
        cls_one[idx >= 0] = 0
        hit = rows[fg]
        cls_one[fg] = 1 if num_class == 1 else hit[:, -1].long()
        cls[mask] = cls_one
        if hit.shape[0] > 0:
            box_one = box.new_zeros((int(mask.sum()), 8))
            box_one[fg] = coder.encode_torch(gt_boxes=hit[:, :-1].clone(), points=pts[fg], gt_classes=hit[:, -1].long())
            box[mask] = box_one
    return cls, box


def numpy_iou3d(rois7, gt7):
    """(M, 7), (G, 7) float32 -> (M, G): the header's volume IoU over tests/rect_overlap_ref.py's footprint overlap (not
    bit-exact to the kernel: its trig is the correctly rounded one).  For the CPU tests."""
    from tests import rect_overlap_ref as ro
    a, b = np.asarray(rois7, F32), np.asarray(gt7, F32)
    M, G = len(a), len(b)
    ai, bi = np.repeat(np.arange(M), G), np.tile(np.arange(G), M)
    over, _ = ro.overlap_area(ro.make_rect(a[ai]), ro.make_rect(b[bi]))
    with np.errstate(all='ignore'):
        half_a, half_b = F32(0.5) * a[ai, 5], F32(0.5) * b[bi, 5]
        z = np.minimum(a[ai, 2] + half_a, b[bi, 2] + half_b) - np.maximum(a[ai, 2] - half_a, b[bi, 2] - half_b)
        inter = over * np.where(z < 0, F32(0), z)
        union = (a[ai, 3] * a[ai, 4] * a[ai, 5] + b[bi, 3] * b[bi, 4] * b[bi, 5]) - inter
        return (inter / np.where(union < F32(1e-6), F32(1e-6), union)).reshape(M, G).astype(F32)


def gpu_iou3d(rois7, gt7):
    from dfu3d_amd.pcdet_kitti import iou3d_nms_utils
    return iou3d_nms_utils.boxes_iou3d_gpu(rois7, gt7)


def cpu_iou3d(rois7, gt7):
    import torch
    return torch.from_numpy(numpy_iou3d(rois7.numpy(), gt7.numpy()))


def plain_max_iou(rois, roi_labels, gt_boxes, by_class, iou_fn):
    """The first half of the reference's per-sample RoI sampling, in its shape: per sample a host read for the cut of the
    trailing all-zero rows, then per class one IoU call between host reads (by_class), or one call and a row maximum.
    -> max_overlaps (B, M), gt_assignment int64 (B, M)."""
    import torch
    B, M = rois.shape[:2]
    ov, asg = rois.new_zeros((B, M)), roi_labels.new_zeros((B, M))
    for b in range(B):
        filled = (gt_boxes[b].sum(dim=1) != 0).nonzero().view(-1)
        n_rows = int(filled.max()) + 1 if filled.numel() else 0           # host read: rows up to the last non-zero one
        if n_rows == 0:
            continue                                                      # nothing to overlap: 0 and row 0
        rows = gt_boxes[b, :n_rows]
        if not by_class:
            ov[b], asg[b] = torch.max(iou_fn(rois[b, :, :7].contiguous(), rows[:, :7].contiguous()), dim=1)
            continue
        row_class = rows[:, -1].long()
        for c in torch.unique(row_class).tolist():                        # host read
            of_rois, of_rows = (roi_labels[b] == c).nonzero().view(-1), (row_class == c).nonzero().view(-1)
            if of_rois.numel() == 0:
                continue
            best, arg = torch.max(iou_fn(rois[b, of_rois, :7].contiguous(), rows[of_rows, :7].contiguous()), dim=1)
            ov[b, of_rois], asg[b, of_rois] = best, of_rows[arg]
    return ov, asg


def plain_subsample(max_overlaps, cfg, rand_key, rand_u):
    """subsample_rois + sample_bg_inds with nonzero, a stable argsort for the permutation prefix and floor(u * n) draws:
    the same rule as the kernel's from array operations.  -> int64 (B, R)."""
    import torch
    R_, fg_per, fg_t, reg_t, lo_t, ratio = sampler_numbers(cfg)
    out = []
    for ov, key, u in zip(max_overlaps, rand_key, rand_u):
        fg = (ov >= float(fg_t)).nonzero().view(-1)
        easy = (ov < float(lo_t)).nonzero().view(-1)
        hard = ((ov < float(reg_t)) & (ov >= float(lo_t))).nonzero().view(-1)
        pick = lambda lst, uu: lst[torch.clamp(torch.floor(uu.double() * lst.numel()).long(), max=lst.numel() - 1)]   # noqa: E731

        def background(uu):
            if hard.numel() > 0 and easy.numel() > 0:
                h = min(int(uu.numel() * ratio), hard.numel())
                return torch.cat((pick(hard, uu[:h]), pick(easy, uu[h:])))
            return pick(hard if hard.numel() > 0 else easy, uu)
        if fg.numel() > 0 and hard.numel() + easy.numel() > 0:
            take = min(fg_per, fg.numel())
            order = torch.argsort(key[fg], stable=True)
            out.append(torch.cat((fg[order[:take]], background(u[take:]))))
        elif fg.numel() > 0:
            out.append(pick(fg, u))
        elif hard.numel() + easy.numel() > 0:
            out.append(background(u))
        else:
            out.append(fg.new_zeros(R_))
    return torch.stack(out)


def plain_proposal_targets(rois, roi_scores, roi_labels, gt_boxes, cfg, sampled_inds, iou_fn):
    """ProposalTargetLayer.forward with the sampled indices given: per-sample indexing, then the labels."""
    import torch
    ov, asg = plain_max_iou(rois, roi_labels, gt_boxes, bool(cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False)), iou_fn)
    B, R_ = sampled_inds.shape
    out = {'rois': rois.new_zeros(B, R_, rois.shape[-1]), 'gt_of_rois': rois.new_zeros(B, R_, gt_boxes.shape[-1]),
           'gt_iou_of_rois': rois.new_zeros(B, R_), 'roi_scores': rois.new_zeros(B, R_),
           'roi_labels': rois.new_zeros((B, R_), dtype=torch.long)}
    for index in range(B):
        s = sampled_inds[index].long()
        out['rois'][index], out['roi_labels'][index] = rois[index][s], roi_labels[index][s]
        out['gt_iou_of_rois'][index], out['roi_scores'][index] = ov[index][s], roi_scores[index][s]
        out['gt_of_rois'][index] = gt_boxes[index][asg[index][s]]
    ious = out['gt_iou_of_rois']
    out['reg_valid_mask'] = (ious > cfg['REG_FG_THRESH']).long()
    if cfg['CLS_SCORE_TYPE'] == 'cls':
        labels = (ious > cfg['CLS_FG_THRESH']).long()
        labels[(ious > cfg['CLS_BG_THRESH']) & (ious < cfg['CLS_FG_THRESH'])] = -1
    else:
        fg, bg = ious > cfg['CLS_FG_THRESH'], ious < cfg['CLS_BG_THRESH']
        between = (fg == 0) & (bg == 0)
        labels = (fg > 0).float()
        labels[between] = (ious[between] - cfg['CLS_BG_THRESH']) / (cfg['CLS_FG_THRESH'] - cfg['CLS_BG_THRESH'])
    out['rcnn_cls_labels'] = labels
    out['max_overlaps'], out['gt_assignment'] = ov, asg
    return out


def plain_roi_targets(targets, batch_size):
    """The second stage's targets after the target layer: 'gt_of_rois_src' keeps the sampled ground truth, 'gt_of_rois' is
    the same box seen from its RoI -- centre relative to the RoI's, turned by minus the RoI's heading (taken modulo 2 pi),
    the heading difference folded into [-pi/2, pi/2] so that a box facing the other way counts as aligned.  Written out
    per column here (the product code goes through rotate_points_along_z).  Returns a new dict."""
    import torch
    out = dict(targets)
    rois, src = targets['rois'], targets['gt_of_rois']
    out['gt_of_rois_src'] = src.clone()
    pi = math.pi
    turn = torch.remainder(rois[..., 6], 2 * pi)
    rel = src[..., 0:3] - rois[..., 0:3]
    c, s = torch.cos(-turn), torch.sin(-turn)
    local_x, local_y = rel[..., 0] * c - rel[..., 1] * s, rel[..., 0] * s + rel[..., 1] * c
    heading = torch.remainder(src[..., 6] - turn, 2 * pi)
    backwards = (heading > 0.5 * pi) & (heading < 1.5 * pi)
    heading = torch.where(backwards, torch.remainder(heading + pi, 2 * pi), heading)
    heading = torch.where(heading > pi, heading - 2 * pi, heading).clamp(min=-pi / 2, max=pi / 2)
    out['gt_of_rois'] = torch.cat((local_x[..., None], local_y[..., None], rel[..., 2:3], src[..., 3:6], heading[..., None],
                                   src[..., 7:]), dim=-1)
    return out


# The losses below are written from their formulas on torch primitives alone: nothing of dfu3d_amd.pcdet_kitti.loss_utils,
# box_utils or box_coder_utils is imported, so they are an independent statement of what the heads must compute.
def _focal_terms(logits, one_hot, alpha=0.25, gamma=2.0):
    """alpha_t (1 - p_t)^gamma BCE(logit, target) per element, p_t the probability of the target."""
    import torch
    import torch.nn.functional as F
    p = torch.sigmoid(logits)
    p_t = torch.where(one_hot > 0, p, 1 - p)
    alpha_t = torch.where(one_hot > 0, torch.full_like(p, alpha), torch.full_like(p, 1 - alpha))
    return alpha_t * (1 - p_t) ** gamma * F.binary_cross_entropy_with_logits(logits, one_hot, reduction='none')


def _huber_terms(pred, target, code_weights, beta=1.0 / 9.0):
    """Smooth L1 with the change point beta of the code-weighted residual; a NaN target costs nothing."""
    import torch
    import torch.nn.functional as F
    target = torch.where(target != target, pred.detach(), target)
    scale = pred.new_tensor(code_weights)
    return F.smooth_l1_loss(pred * scale, target * scale, reduction='none', beta=beta)


def _corners(boxes):
    """(n, 7) -> (n, 8, 3): centre + Rz(heading) (sign * dims / 2), bottom face first, each face counter-clockwise from
    (+, +)."""
    import torch
    sign = boxes.new_tensor([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]])
    off = 0.5 * boxes[:, None, 3:6] * sign[None]
    c, s = torch.cos(boxes[:, 6])[:, None], torch.sin(boxes[:, 6])[:, None]
    return torch.stack((boxes[:, None, 0] + off[..., 0] * c - off[..., 1] * s, boxes[:, None, 1] + off[..., 0] * s + off[..., 1] * c,
                        boxes[:, None, 2] + off[..., 2]), dim=-1)


def _corner_terms(pred7, gt7):
    """(n): the mean over the corners of the Huber (beta 1) distance to the nearer of the box and the box turned by pi."""
    import torch
    import torch.nn.functional as F
    turned = torch.cat((gt7[:, :6], gt7[:, 6:7] + math.pi), dim=1)
    pc = _corners(pred7)
    dist = torch.minimum((pc - _corners(gt7)).pow(2).sum(-1).sqrt(), (pc - _corners(turned)).pow(2).sum(-1).sqrt())
    return F.smooth_l1_loss(dist, torch.zeros_like(dist), reduction='none', beta=1.0).mean(dim=1)


def plain_point_losses(cls_preds, box_preds, cls_labels, box_labels, num_class, weights, code_weights):
    """The first stage's two losses -> {'point_loss_cls', 'point_loss_box', 'point_pos_num'} (0-dim tensors) and the
    per-element terms 'cls_terms' (N, num_class), 'box_terms' (N, 8): focal loss of every point that is not ignored against
    the one-hot of its class, smooth L1 of the positives' codes, both divided by the number of positives (at least 1)."""
    import torch
    import torch.nn.functional as F
    labels = cls_labels.view(-1)
    n_pos = (labels > 0).sum().float()
    norm = n_pos.clamp(min=1.0)
    one_hot = F.one_hot(labels.clamp(min=0), num_class + 1)[:, 1:].to(cls_preds.dtype)
    cls_terms = _focal_terms(cls_preds.view(-1, num_class), one_hot) * ((labels >= 0).float() / norm)[:, None]
    box_terms = _huber_terms(box_preds, box_labels, code_weights) * ((labels > 0).float() / norm)[:, None]
    return {'point_loss_cls': cls_terms.sum() * weights['point_cls_weight'], 'point_pos_num': n_pos,
            'point_loss_box': box_terms.sum() * weights['point_box_weight'], 'cls_terms': cls_terms, 'box_terms': box_terms}


def plain_rcnn_losses(ret, code_size, loss_cfg):
    """The second stage's losses with the foreground rows picked by boolean indexing and the corner term behind a host
    read of their number (the reference's shape).  ret: rcnn_cls, rcnn_reg, rcnn_cls_labels, reg_valid_mask, gt_of_rois,
    gt_of_rois_src, rois.  -> {'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'} (0-dim tensors) and
    'reg_terms' (rows, 7), the smooth L1 of every row before the mask."""
    import torch
    import torch.nn.functional as F
    w = loss_cfg['LOSS_WEIGHTS']
    labels = ret['rcnn_cls_labels'].view(-1)
    keep = labels >= 0
    if loss_cfg['CLS_LOSS'] == 'BinaryCrossEntropy':
        each = F.binary_cross_entropy_with_logits(ret['rcnn_cls'].view(-1)[keep], labels[keep].float(), reduction='none')
    else:
        each = F.cross_entropy(ret['rcnn_cls'][keep], labels[keep], reduction='none')
    loss_cls = each.sum() / max(int(keep.sum()), 1) * w['rcnn_cls_weight']
    fg = ret['reg_valid_mask'].view(-1) > 0
    n_fg = int(fg.sum())                                                  # host read
    rois = ret['rois'].reshape(-1, code_size).detach()
    gt_ct = ret['gt_of_rois'][..., 0:code_size].reshape(-1, code_size)
    gt_src = ret['gt_of_rois_src'][..., 0:code_size].reshape(-1, code_size)
    reg = ret['rcnn_reg'].view(rois.shape[0], -1)
    size = rois[:, 3:6].clamp(min=1e-5)
    diag = (size[:, 0] ** 2 + size[:, 1] ** 2).sqrt()
    target = torch.cat((gt_ct[:, 0:1] / diag[:, None], gt_ct[:, 1:2] / diag[:, None], gt_ct[:, 2:3] / size[:, 2:3],
                        (gt_ct[:, 3:6].clamp(min=1e-5) / size).log(), gt_ct[:, 6:7]), dim=1)          # the anchor: heading 0
    reg_terms = _huber_terms(reg, target, w['code_weights'])
    loss_reg = reg_terms[fg].sum() / max(n_fg, 1) * w['rcnn_reg_weight']
    corner = loss_reg.new_zeros(())
    if loss_cfg['CORNER_LOSS_REGULARIZATION'] and n_fg > 0:
        r, t, sz, dg = rois[fg], reg[fg], size[fg], diag[fg]
        lx, ly, lz = t[:, 0] * dg, t[:, 1] * dg, t[:, 2] * sz[:, 2]
        c, s = torch.cos(r[:, 6]), torch.sin(r[:, 6])
        boxes = torch.stack((lx * c - ly * s + r[:, 0], lx * s + ly * c + r[:, 1], lz + r[:, 2], t[:, 3].exp() * sz[:, 0],
                             t[:, 4].exp() * sz[:, 1], t[:, 5].exp() * sz[:, 2], t[:, 6] + r[:, 6]), dim=1)
        corner = _corner_terms(boxes, gt_src[fg][:, 0:7]).mean() * w['rcnn_corner_weight']
    return {'rcnn_loss_cls': loss_cls, 'rcnn_loss_reg': loss_reg, 'rcnn_loss_corner': corner,
            'rcnn_loss': loss_cls + loss_reg + corner, 'reg_terms': reg_terms}


# ---- cases ------------------------------------------------------------------------------------------------------------
MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
SAMPLER = {'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls',
           'CLS_FG_THRESH': 0.6, 'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}


def random_boxes(rng, B, G, classes=3, spread=6.0):
    """(B, G, 8): boxes of 0.6 .. 5 m within +-spread with headings over all four quadrants and classes 1 .. classes."""
    gt = np.zeros((B, G, 8), F32)
    gt[..., :2] = rng.uniform(-spread, spread, (B, G, 2))
    gt[..., 2] = rng.uniform(-1.0, 1.0, (B, G))
    gt[..., 3:6] = rng.uniform(0.6, 5.0, (B, G, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (B, G))
    gt[..., 7] = rng.integers(1, classes + 1, (B, G))
    return gt


def random_point_case(seed, B, N, G):
    """Clouds within +-8 m of which a third is drawn inside (or just around) a box of the sample."""
    rng = np.random.default_rng(seed)
    gt = random_boxes(rng, B, G)
    pts = rng.uniform(-8.0, 8.0, (B, N, 3)).astype(F32)
    pts[..., 2] *= F32(0.25)
    for b in range(B):
        for n in range(0, N, 3):
            g = int(rng.integers(0, G))
            local = rng.uniform(-0.56, 0.56, 3) * gt[b, g, 3:6]
            c, s = np.cos(gt[b, g, 6]), np.sin(gt[b, g, 6])
            pts[b, n] = gt[b, g, :3] + np.array([local[0] * c - local[1] * s, local[0] * s + local[1] * c, local[2]])
    return pts, gt


def jittered_rois(rng, gt, M):
    """(B, M, 7) RoIs: ground-truth boxes of the sample moved, resized and turned a little (every level of IoU), labels
    int64 (B, M) mostly the box's class."""
    B, G = gt.shape[:2]
    rois, labels = np.zeros((B, M, 7), F32), np.zeros((B, M), np.int64)
    for b in range(B):
        for m in range(M):
            g = int(rng.integers(0, G))
            scale = rng.choice([0.02, 0.1, 0.3, 1.0])
            rois[b, m] = gt[b, g, :7]
            rois[b, m, :3] += rng.normal(0, 0.5, 3) * scale
            rois[b, m, 3:6] *= 1.0 + rng.uniform(-0.3, 0.3, 3) * scale
            rois[b, m, 6] += rng.normal(0, 0.3) * scale
            labels[b, m] = int(gt[b, g, 7]) if rng.uniform() < 0.8 or gt[b, g, 7] < 1 else int(rng.integers(1, 4))
    return rois, labels


def same_bits(a, b):
    return R.same_bits(a, b)
