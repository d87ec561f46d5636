/* Shadows the reference header of the same name: temporary file names and
   path clean-up for the loaders in MatchList.h. */
#ifndef MUMS_REF_SHIM_FILES_H
#define MUMS_REF_SHIM_FILES_H
#include <stdio.h>
#include <unistd.h>
#include <string>
#include <vector>

inline std::string CreateTempFileName(const std::string& prefix) {
	static unsigned serial = 0;
	const char* dir = getenv("TMPDIR");
	char buf[64];
	snprintf(buf, sizeof buf, "%ld_%u", (long)getpid(), serial++);
	return std::string(dir ? dir : "/tmp") + "/" + prefix + buf;
}

inline void standardizePath(std::string&) {}

inline std::vector<std::string>& registerFileToDelete(std::string fname = "") {
	static std::vector<std::string> files;
	if (!fname.empty())
		files.push_back(fname);
	return files;
}

inline void deleteRegisteredFiles() {
	std::vector<std::string>& files = registerFileToDelete();
	for (size_t i = 0; i < files.size(); i++)
		remove(files[i].c_str());
	files.clear();
}
#endif
