"""Where the training scripts' scalars go (superpoint_train_descriptor.py, superpoint_glue_train.py): tensorboardX's SummaryWriter where
that package is installed, otherwise one JSON line per add_scalar in <dir>/scalars.jsonl."""
import json
import logging
import os


class JsonlWriter:
    """add_scalar(tag, value, step) -> one JSON line: what stands in for tensorboardX.SummaryWriter where it is not installed"""

    def __init__(self, path):
        self.f = open(path, "a")

    def add_scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self.f.flush()

    def close(self):
        self.f.close()


def make_writer(output_dir):
    try:
        from tensorboardX import SummaryWriter
        return SummaryWriter(output_dir)
    except ImportError:
        os.makedirs(output_dir, exist_ok=True)
        logging.info("tensorboardX is not installed: scalars go to %s", os.path.join(output_dir, "scalars.jsonl"))
        return JsonlWriter(os.path.join(output_dir, "scalars.jsonl"))
