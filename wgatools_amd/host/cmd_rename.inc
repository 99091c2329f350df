/* cmd_rename.inc — part of wgatools_main.cpp (included there, inside its namespace: the commands share the device helpers, readers and
 * writers defined in front of the include). */
/* ---- rename (tools/rename.rs, MAFRecord::rename maf.rs:250-261, utils.rs:579-591) ---------------------------------------------
 * Row r of every block gets prefix r in front of its name: K22 (wga_maf_rewrite) with the prefixes uploaded once per device and
 * no filter; pieces, windows and --gpus N are rewrite_maf's (cmd_filter.inc).  A block whose row count differs from the number
 * of prefixes ends the output in front of it (errors.rs:77). */
int cmd_rename(const std::string* input, const std::vector<std::string>& prefixes, Output& out) {
  MafRewrite rw;
  rw.prefixes = prefixes;
  rw.bad_message = "S-line count not match";
  std::string header = "#maf version=1.6 rename=";
  for (size_t k = 0; k < prefixes.size(); k++) header += (k ? ";" : "") + prefixes[k];
  return rewrite_maf(input, header, rw, out);
}
