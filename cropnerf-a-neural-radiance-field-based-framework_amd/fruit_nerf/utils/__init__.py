"""Data preparation commands: convert_segmentation_img_to_label."""
