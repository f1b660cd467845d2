"""`import utils` (train.py:9, generate_frames.py:9): the path-relevant helpers of the reference's
utils.py, restated in dvg_amd/utils.py; its image / GIF writers compose their figures on the device (dvg_amd/viz.py), its
finn_eval_seq is computed there (dvg_eval_frames_finn), and so is sample_diversity (dvg_pairwise_frame_mse; no counterpart in the reference)."""
from dvg_amd.utils import (add_border, draw_text_tensor, finn_eval_seq, image_tensor, init_weights, normalize_data,  # noqa: F401
                           sample_diversity, save_gif, save_gif_with_text, save_tensors_image)
