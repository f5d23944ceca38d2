"""tools/eval_utils/eval_utils.py (the writer of the self-evolution loop): one evaluation epoch of a
detector over `KittiDataset.batches(...)` -- the model under torch.no_grad(), the recall record, the KITTI annotation
dictionaries (and result files with args.save_to_file), result.pkl, the official AP report.

`dataloader` is the Batches object; `dataloader.dataset` the KittiDataset.  The batches are on the device already, so
there is no load_data_to_gpu.  cfg: MODEL.POST_PROCESSING.RECALL_THRESH_LIST and EVAL_METRIC, optionally LOCAL_RANK
(default 0), as a dict or an attribute object.  Divergences: dist_test=True raises
NotImplementedError, as the training loop refuses DistributedDataParallel; no progress bar; result.pkl is written (the
reference's copy has the two lines commented out)."""
import pickle
import time
from pathlib import Path

import torch

from ..pcdet_kitti.centerpoint import _get


def _thresholds(cfg):
    return _get(_get(_get(cfg, 'MODEL'), 'POST_PROCESSING'), 'RECALL_THRESH_LIST')


def statistics_info(cfg, ret_dict, metric, disp_dict):
    """eval_utils.py:12-19: the batch's recall record added to the epoch's."""
    thresholds = _thresholds(cfg)
    for cur_thresh in thresholds:
        metric['recall_roi_%s' % str(cur_thresh)] += ret_dict.get('roi_%s' % str(cur_thresh), 0)
        metric['recall_rcnn_%s' % str(cur_thresh)] += ret_dict.get('rcnn_%s' % str(cur_thresh), 0)
    metric['gt_num'] += ret_dict.get('gt', 0)
    min_thresh = thresholds[0]
    disp_dict['recall_%s' % str(min_thresh)] = '(%d, %d) / %d' % (
        metric['recall_roi_%s' % str(min_thresh)], metric['recall_rcnn_%s' % str(min_thresh)], metric['gt_num'])


def eval_one_epoch(cfg, args, model, dataloader, epoch_id, logger, dist_test=False, result_dir=None):
    """eval_utils.py:22-136 -> ret_dict: 'recall/roi_<t>', 'recall/rcnn_<t>' for every threshold and the AP dictionary."""
    if dist_test:
        raise NotImplementedError("eval_one_epoch: dist_test (DistributedDataParallel, merge_results_dist) is not supported")
    result_dir = Path(result_dir)
    result_dir.mkdir(parents=True, exist_ok=True)
    final_output_dir = result_dir / 'final_result' / 'data'
    save_to_file = bool(_get(args, 'save_to_file', False))
    if save_to_file:
        final_output_dir.mkdir(parents=True, exist_ok=True)

    thresholds = _thresholds(cfg)
    metric = {'gt_num': 0}
    for cur_thresh in thresholds:
        metric['recall_roi_%s' % str(cur_thresh)] = 0
        metric['recall_rcnn_%s' % str(cur_thresh)] = 0

    dataset = dataloader.dataset
    class_names = dataset.class_names
    det_annos = []

    logger.info('*************** EPOCH %s EVALUATION *****************' % epoch_id)
    model.eval()
    start_time = time.time()
    for batch_dict in dataloader:
        with torch.no_grad():
            pred_dicts, ret_dict = model(batch_dict)
        disp_dict = {}
        statistics_info(cfg, ret_dict, metric, disp_dict)
        det_annos += dataset.generate_prediction_dicts(batch_dict, pred_dicts, class_names,
                                                       output_path=final_output_dir if save_to_file else None)

    logger.info('*************** Performance of EPOCH %s *****************' % epoch_id)
    sec_per_example = (time.time() - start_time) / max(len(dataset), 1)
    logger.info('Generate label finished(sec_per_example: %.4f second).' % sec_per_example)
    if _get(cfg, 'LOCAL_RANK', 0) != 0:
        return {}

    ret_dict = {}
    gt_num_cnt = metric['gt_num']
    for cur_thresh in thresholds:
        cur_roi_recall = metric['recall_roi_%s' % str(cur_thresh)] / max(gt_num_cnt, 1)
        cur_rcnn_recall = metric['recall_rcnn_%s' % str(cur_thresh)] / max(gt_num_cnt, 1)
        logger.info('recall_roi_%s: %f' % (cur_thresh, cur_roi_recall))
        logger.info('recall_rcnn_%s: %f' % (cur_thresh, cur_rcnn_recall))
        ret_dict['recall/roi_%s' % str(cur_thresh)] = cur_roi_recall
        ret_dict['recall/rcnn_%s' % str(cur_thresh)] = cur_rcnn_recall

    total_pred_objects = sum(len(anno['name']) for anno in det_annos)
    logger.info('Average predicted number of objects(%d samples): %.3f'
                % (len(det_annos), total_pred_objects / max(1, len(det_annos))))

    with open(result_dir / 'result.pkl', 'wb') as f:
        pickle.dump(det_annos, f)

    result_str, result_dict = dataset.evaluation(
        det_annos, class_names, eval_metric=_get(_get(_get(cfg, 'MODEL'), 'POST_PROCESSING'), 'EVAL_METRIC', 'kitti'),
        output_path=final_output_dir)
    logger.info(result_str)
    ret_dict.update(result_dict)

    logger.info('Result is saved to %s' % result_dir)
    logger.info('****************Evaluation done.*****************')
    return ret_dict
