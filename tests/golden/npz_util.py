"""A reproducible .npz writer for the fixture generators: numpy's own savez stamps every member with the current time, so
two runs of a generator differ byte for byte; here members carry a fixed date, are written in sorted key order and
deflated at a fixed level."""
import io
import zipfile

import numpy as np


def save_npz(path, **arrays):
    with zipfile.ZipFile(path, "w") as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
