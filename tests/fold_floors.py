"""Measured figures (whole tensor, worst slice) of the restatements of fold_refs.py against fp64, on the CPU: the per-slice bounds of
test_ff_fold_gpu.py are computed from them (fold_refs.bounds); test_ff_fold_host.py measures them again.  Regenerate: python tests/fold_refs.py"""
FLOORS = {
    "compose/64/bf16:b": (7.984e-08, 1.754e-07),
    "compose/128/bf16:b": (7.187e-08, 1.661e-07),
    "compose/88/bf16:b": (6.784e-08, 1.633e-07),
    "tail/64x64/bf16:y": (1.817e-03, 2.344e-03),
    "tail/192x64/bf16:y": (1.864e-03, 2.301e-03),
    "tail/64x128/bf16:y": (1.993e-03, 2.463e-03),
    "tail/192x128/bf16:y": (1.937e-03, 2.300e-03),
    "compose/64/fp16:b": (6.393e-08, 1.459e-07),
    "compose/128/fp16:b": (6.368e-08, 1.628e-07),
    "compose/88/fp16:b": (6.273e-08, 2.067e-07),
    "tail/64x64/fp16:y": (2.166e-04, 3.058e-04),
    "tail/192x64/fp16:y": (2.347e-04, 2.896e-04),
    "tail/64x128/fp16:y": (2.402e-04, 2.904e-04),
    "tail/192x128/fp16:y": (2.382e-04, 2.871e-04),
}
