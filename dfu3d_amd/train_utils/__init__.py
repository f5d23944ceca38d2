"""tools/train_utils of the reference on this package's HIP stages: `optimization` (build_optimizer, build_scheduler, the
fused OptimWrapper, the one-cycle schedules) and `train_utils` (train_one_epoch, train_model, checkpoints)."""
