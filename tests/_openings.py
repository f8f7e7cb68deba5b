"""The column-opening section of a proof stream, built from the oracle's rows and trees (shared by the GPU parity tests)."""
import numpy as np


def _expected_openings(z, rows_o, layers_o, cols):
    """The column-opening section of the proof stream from the oracle's rows and trees (open_z.rs:124-143,
    pcs/utils.rs:163-176): per opening the column's values, then per row be64(depth) + the siblings, leaf level first."""
    R, cw, d = z.num_rows, z.codeword_len, z.depth
    rows3 = np.ascontiguousarray(rows_o.reshape(R, cw, 4).astype("<u8")).view(np.uint8).reshape(R, cw, 32)
    out = np.zeros((len(cols), R * (32 + 8 + 32 * d)), dtype=np.uint8)
    hdr = np.frombuffer(int(d).to_bytes(8, "big"), dtype=np.uint8)
    for i, c in enumerate(int(c) for c in cols):
        out[i, : R * 32] = rows3[:, c, :].reshape(-1)
        rec = out[i, R * 32:].reshape(R, 8 + 32 * d)
        rec[:, :8] = hdr
        for k in range(d):
            rec[:, 8 + 32 * k: 40 + 32 * k] = layers_o[:, 2 * cw - ((2 * cw) >> k) + ((c >> k) ^ 1), :]
    return out.reshape(-1)
