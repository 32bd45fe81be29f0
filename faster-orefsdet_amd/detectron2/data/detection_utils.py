"""d2z:data/detection_utils.py: the image reader the demo and the mappers use.  Pillow decodes; the array is what the model's raw-image
request takes ([h, w, 3] uint8 for "RGB" / "BGR")."""
import numpy as np

__all__ = ["read_image"]


def read_image(file_name, format=None):
    """Read an image into a numpy array: "RGB" and "BGR" give [h, w, 3] uint8, "L" gives [h, w, 1] uint8 (detectron2's
    convert_PIL_to_numpy keeps the channel axis of a grey image), None keeps the file's own mode as Pillow reports it.  An EXIF
    orientation tag is applied first, as upstream does (a photo taken with the camera turned comes out upright); a file without
    the tag is returned as stored."""
    from PIL import Image, ImageOps
    if format not in (None, "RGB", "BGR", "L"):
        raise ValueError(f'read_image: format is "RGB", "BGR", "L" or None, not {format!r}')
    with open(file_name, "rb") as f:
        image = ImageOps.exif_transpose(Image.open(f))
        if format is not None:
            image = image.convert("RGB" if format == "BGR" else format)
        image = np.asarray(image)
    if format == "BGR":
        return np.ascontiguousarray(image[:, :, ::-1])
    if format == "L":
        return np.expand_dims(image, -1)
    return image
