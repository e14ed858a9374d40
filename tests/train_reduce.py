"""The average omok_train_apply forms from the ranks' gradient slabs, restated in numpy fp32 (a helper of the tests, not a test):
per element g = s[0]; g += s[r] for r = 1 .. R - 1 in rank order; g *= 1.0f / (float)R.  Every operation is one IEEE fp32 operation
(numpy keeps float32 operands in float32, subnormals included), so the result is the bit pattern the kernel must leave."""
import numpy as np


def average(slabs):
    """slabs: [R, count] (or a list of R arrays) -> their rank-order fp32 average [count]"""
    slabs = [np.asarray(s, np.float32) for s in slabs]
    g = slabs[0].copy()
    for s in slabs[1:]:
        g = g + s
    return g * (np.float32(1) / np.float32(len(slabs)))
