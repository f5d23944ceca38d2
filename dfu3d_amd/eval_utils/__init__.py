"""tools/eval_utils of the reference: the evaluation epoch over KittiDataset.batches (eval_utils.eval_one_epoch)."""
